"""CPU tests of the bitstream file (gsvc_amd/bitstream.py) and of what the picture hash does before a launch: the section framing on
synthetic payloads, typed header fields bit for bit, unknown sections, every truncation and every flipped byte named by its section,
the argument checks of gsvc_picture_hash, and the NumPy statement of the hash (tests/_picture_hash_ref.py) on values done by hand."""
import struct
import zlib

import numpy as np
import pytest
import torch

from gsvc_amd import _lib, bitstream as B, metrics
from gsvc_amd.frames_out import FrameFormat, frame_bytes
from gsvc_amd.stream_codec import StreamPack
from tests import _picture_hash_ref as ref


# ---- framing ----------------------------------------------------------------------------------------------------------------------
def _payloads():
    rng = np.random.default_rng(7)
    return [(b"HEAD", rng.bytes(41)), (b"MLPS", rng.bytes(1000)), (b"ANCH", b""), (b"MASK", rng.bytes(1)), (b"SLAB", rng.bytes(257))]


def test_sections_round_trip():
    sections = _payloads()
    blob = B.pack_sections(sections)
    assert blob[:4] == b"GSVC" and struct.unpack_from("<HH", blob, 4) == (1, len(sections))
    assert len(blob) == 8 + 16 * len(sections) + sum(len(p) for _, p in sections)
    assert B.unpack_sections(blob) == sections
    tag, length, crc = struct.unpack_from("<4sQI", blob, 8 + 16)
    assert (tag, length, crc) == (b"MLPS", 1000, zlib.crc32(sections[1][1]))


def test_unknown_sections_are_skipped():
    sections = _payloads()
    blob = B.pack_sections(sections[:2] + [(b"XTRA", b"from a later version")] + sections[2:])
    assert [t for t, _ in B.unpack_sections(blob)] == [b"HEAD", b"MLPS", b"XTRA", b"ANCH", b"MASK", b"SLAB"]
    assert B.unpack_sections(blob, known=B.KNOWN_TAGS) == sections


def test_header_fields_come_back_bit_for_bit():
    fields = {"an_int": -5, "big": 2 ** 40 + 3, "yes": True, "no": False, "tiny": 1e-19, "tenth": float(np.float32(0.1)), "as_f32": np.float32(0.1),
              "neg_zero": -0.0, "text": "yuv420p10le", "ints": [18, 24, 33], "no_ints": [], "floats": [1e-19, 0.1, -2.5],
              "array": np.array([0.001, 1e30], np.float32), "slabs": (0, 7, 7, 9)}
    back = B.unpack_fields(B.pack_fields(fields))
    assert list(back) == list(fields)
    assert back["an_int"] == -5 and back["big"] == 2 ** 40 + 3 and back["yes"] is True and back["no"] is False
    assert back["text"] == "yuv420p10le" and back["ints"] == (18, 24, 33) and back["no_ints"] == () and back["slabs"] == (0, 7, 7, 9)
    for name, want in (("tiny", 1e-19), ("tenth", 0.1), ("as_f32", 0.1), ("neg_zero", -0.0)):
        assert isinstance(back[name], np.float32) and back[name].tobytes() == np.float32(want).tobytes(), name
    assert float(back["tiny"]) != 0.0 and np.signbit(back["neg_zero"])
    assert np.asarray(back["floats"], np.float32).tobytes() == np.array([1e-19, 0.1, -2.5], np.float32).tobytes()
    assert np.asarray(back["array"], np.float32).tobytes() == fields["array"].tobytes()
    assert B.pack_fields(back) == B.pack_fields(fields)          # (a second trip changes nothing)
    with pytest.raises(TypeError):
        B.pack_fields({"bad": object()})
    with pytest.raises(B.BitstreamError, match="HEAD"):
        B.unpack_fields(B.pack_fields(fields)[:-3])


# ---- a whole file on a synthetic pack -------------------------------------------------------------------------------------------------
class _Shape:
    """What ``make_header`` reads of a model."""
    feat_dim, n_offsets, voxel_size, update_depth, update_init_factor, update_hierachy_factor = 50, 10, 0.001, 3, 16, 4
    n_features_per_level, log2_hashmap_size, log2_hashmap_size_2D = 8, 13, 15
    resolutions_list, resolutions_list_2D = (18, 24, 33, 44), (130, 258)
    use_2D, ste_binary, ste_multistep, add_noise, Q = True, True, False, False, 1
    x_bound_min, x_bound_max = torch.tensor([[-1.1, -0.825, -0.1375]]), torch.tensor([[1.1, 0.825, 0.1375]])

    class model_config:
        time_multi_res, offset_multi_res = 16, 16


def _file(hashes=True):
    rng = np.random.default_rng(11)
    pack = StreamPack(n_full=1200, n=1000, anchor_interval=np.array([3e-5, 2e-5, 1e-5], np.float32), anchor_min=np.array([-1.1, -0.8, -0.1], np.float32),
                      anchors_q=None, prob_masks=float(np.float32(0.37)), prob_hash=float(np.float32(0.501)), slabs=[(0, 400), (400, 1000)],
                      feat=[rng.bytes(300), rng.bytes(211)], scaling=[rng.bytes(90), rng.bytes(77)], offsets=[rng.bytes(120), b""],
                      masks=rng.bytes(64), hash=rng.bytes(500), anchor_stream=rng.bytes(333))
    geo = B.CubeGeometry(W=64, H=48, frames=8, scale=32.0, x_min=-1.0, y_min=-0.75, z_min=-0.125, threshold=0.125, fps=(30000, 1001))
    fmt = FrameFormat("yuv420p", depth=10)
    h = rng.integers(0, 2 ** 63, (8, 3), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    mlp = rng.bytes(800)
    return B.bitstream_bytes(_Shape, pack, geo, mlp, (fmt, h) if hashes else None), pack, geo, mlp, fmt, h


def test_file_round_trip_on_synthetic_streams(tmp_path):
    blob, pack, geo, mlp, fmt, h = _file()
    path = tmp_path / "clip.gsvc"
    path.write_bytes(blob)
    bs = B.read_bitstream(path)
    assert bs.file_bytes == len(blob) and sum(bs.section_bytes.values()) + 8 + 16 * 7 == len(blob)
    assert bs.mlp_bytes == mlp and bs.pack.anchor_stream == pack.anchor_stream and bs.pack.masks == pack.masks and bs.pack.hash == pack.hash
    assert bs.pack.feat == pack.feat and bs.pack.scaling == pack.scaling and bs.pack.offsets == pack.offsets
    assert bs.pack.slabs == pack.slabs and (bs.pack.n_full, bs.pack.n) == (1200, 1000)
    assert bs.pack.prob_masks == pack.prob_masks and bs.pack.prob_hash == pack.prob_hash
    assert bs.pack.anchor_interval.tobytes() == pack.anchor_interval.tobytes() and bs.pack.anchor_min.tobytes() == pack.anchor_min.tobytes()
    assert np.asarray(bs.header["x_bound_min"], np.float32).tobytes() == _Shape.x_bound_min.numpy().tobytes()
    assert bs.geometry == geo and bs.header["resolutions_list"] == (18, 24, 33, 44) and bs.header["fps_num"] == 30000
    assert bs.hash_format == FrameFormat("yuv420p", depth=10, rounding="nearest") and bs.hashes.dtype == np.uint64 and np.array_equal(bs.hashes, h)
    plain = B.parse_bitstream(_file(hashes=False)[0])
    assert plain.hashes is None and plain.hash_format is None
    frames = bs.frames()
    assert len(frames) == 8 and frames[3].z == (3 - 4) / 32.0 and frames[0].image is None and frames[0].image_width == 64


def _table(blob):
    count = struct.unpack_from("<H", blob, 6)[0]
    at, out = 8 + 16 * count, []
    for i in range(count):
        tag, length, _ = struct.unpack_from("<4sQI", blob, 8 + 16 * i)
        out.append((tag.decode(), at, length))
        at += length
    return out


def test_truncation_at_every_section_boundary_names_the_section():
    blob = _file()[0]
    table = _table(blob)
    assert [t for t, _, _ in table] == ["HEAD", "MLPS", "ANCH", "MASK", "HASH", "SLAB", "PHSH"]
    for k, (tag, start, length) in enumerate(table):
        for cut in (start, start + length - 1):          # the section is absent; its last byte is
            with pytest.raises(B.BitstreamError) as e:
                B.parse_bitstream(blob[:cut])
            assert e.value.section == tag and tag in str(e.value), (tag, cut)
    for cut, where in ((0, "magic"), (3, "magic"), (6, "version"), (8, "table"), (8 + 16 * 7 - 1, "table")):
        with pytest.raises(B.BitstreamError) as e:
            B.parse_bitstream(blob[:cut])
        assert e.value.section == where, cut


def test_a_flipped_payload_byte_names_the_section():
    blob = _file()[0]
    for tag, start, length in _table(blob):
        for at in (start, start + length // 2, start + length - 1):
            bad = bytearray(blob)
            bad[at] ^= 0x40
            with pytest.raises(B.BitstreamError, match="CRC") as e:
                B.parse_bitstream(bytes(bad))
            assert e.value.section == tag, (tag, at)


def test_bad_magic_newer_version_and_missing_sections():
    blob = _file()[0]
    with pytest.raises(B.BitstreamError) as e:
        B.parse_bitstream(b"GSVX" + blob[4:])
    assert e.value.section == "magic"
    with pytest.raises(B.BitstreamError, match="version 2") as e:
        B.parse_bitstream(blob[:4] + struct.pack("<H", 2) + blob[6:])
    assert e.value.section == "version"
    sections = B.unpack_sections(blob)
    with pytest.raises(B.BitstreamError) as e:
        B.parse_bitstream(B.pack_sections([s for s in sections if s[0] != b"MASK"]))
    assert e.value.section == "MASK" and "missing" in str(e.value)
    with pytest.raises(B.BitstreamError) as e:          # a SLAB section with a stream too few for the header's two slabs
        B.parse_bitstream(B.pack_sections([(t, p[:-8] if t == b"SLAB" else p) for t, p in sections]))
    assert e.value.section == "SLAB"
    with pytest.raises(B.BitstreamError) as e:          # hashes of 7 frames in a file of 8
        B.parse_bitstream(B.pack_sections([(t, B._pack_hashes(FrameFormat("yuv420p"), np.zeros((7, 3), np.uint64)) if t == b"PHSH" else p)
                                           for t, p in sections]))
    assert e.value.section == "PHSH"
    with pytest.raises(ValueError, match="float32"):
        pack = _file()[1]
        pack.prob_masks = 0.37
        B.bitstream_bytes(_Shape, pack, _file()[2], b"")


# ---- the picture hash ---------------------------------------------------------------------------------------------------------------
def _mix_by_hand(s, c):
    x = ((s * 0x9E3779B1) ^ ((c + 1) * 0x85EBCA6B)) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
    x ^= x >> 12
    return x


def test_reference_on_a_2x2_plane_by_hand():
    """Python integers masked to 32 bits against the uint32 arrays; the first term written out step by step: s = 0, c = 0 starts at
    x = 0 ^ 1 * 0x85EBCA6B, whose upper 17 bits are 0x10BD7."""
    x = 0x85EBCA6B
    x ^= x >> 15
    assert x == 0x85EBCA6B ^ 0x00010BD7
    x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
    x ^= x >> 12
    assert int(ref.mix([0], [0])[0]) == x == _mix_by_hand(0, 0)
    codes = [7, 0, 255, 16]
    want = sum(_mix_by_hand(s, c) for s, c in enumerate(codes))
    assert ref.plane_hash(np.array(codes, np.uint8)) == want and want > 2 ** 32
    # a 2 x 2 4:2:0 frame: Y = the four codes, U = 128, V = 64, each chroma plane one sample at s = 0
    frame = np.array([codes + [128, 64]], np.uint8)
    assert ref.picture_hash_ref(frame, 2, 2, "yuv420p", 8).tolist() == [[want, _mix_by_hand(0, 128), _mix_by_hand(0, 64)]]
    # rgb24, 1 x 2: the plane is the channel, s the pixel
    rgb = np.array([[1, 2, 3, 4, 5, 6]], np.uint8)
    assert ref.picture_hash_ref(rgb, 1, 2, "rgb24", 8).tolist() == [[_mix_by_hand(0, 1) + _mix_by_hand(1, 4), _mix_by_hand(0, 2) + _mix_by_hand(1, 5),
                                                                   _mix_by_hand(0, 3) + _mix_by_hand(1, 6)]]
    # 16-bit words, little-endian: code 0xFFFF
    deep = np.array([[0xFF, 0xFF] * 12], np.uint8)
    assert ref.picture_hash_ref(deep, 2, 2, "yuv444p", 16).tolist() == [[sum(_mix_by_hand(s, 65535) for s in range(4))] * 3]


def test_swapping_two_unequal_samples_changes_the_hash():
    rng = np.random.default_rng(2)
    plane = rng.integers(0, 256, 60, dtype=np.uint8)
    base = ref.plane_hash(plane)
    for i, j in ((0, 1), (3, 59), (20, 21)):
        assert plane[i] != plane[j]
        swapped = plane.copy()
        swapped[[i, j]] = plane[[j, i]]
        assert sorted(swapped) == sorted(plane) and ref.plane_hash(swapped) != base
    assert ref.plane_hash(plane.copy()) == base


def test_hash_entry_point_validates_on_the_host():
    L = _lib.lib()
    ok = (64, 48, 1, 4, 4, 0, 8, 256, None)          # frames, stride, n, H, W, layout, depth, out, stream
    cases = [((None,) + ok[1:], b"NULL"), (ok[:7] + (None, None), b"NULL"), (ok[:2] + (0,) + ok[3:], b"n must be"),
             (ok[:5] + (3,) + ok[6:], b"unknown layout"), (ok[:5] + (-1,) + ok[6:], b"unknown layout"), (ok[:6] + (7,) + ok[7:], b"depth must be"),
             (ok[:6] + (17,) + ok[7:], b"depth must be"), (ok[:6] + (10,) + ok[7:], b"rgb24 frames are 8-bit"),
             ((64, 48, 1, 3, 4, 2, 8, 256, None), b"even"), ((64, 48, 1, 4, 3, 2, 8, 256, None), b"even"),
             ((64, 47, 1, 4, 4, 0, 8, 256, None), b"shorter than a frame"), ((65, 96, 1, 4, 4, 1, 10, 256, None), b"2-byte aligned"),
             ((64, 97, 1, 4, 4, 1, 10, 256, None), b"multiple of 2"), ((64, 95, 1, 4, 4, 1, 10, 256, None), b"shorter than a frame"),
             ((64, 48, 1, 0, 4, 0, 8, 256, None), b"image size"), ((64, 48, 1, 4, 4, 0, 8, 260, None), b"8-byte aligned")]
    for args, msg in cases:
        assert L.gsvc_picture_hash(*args) == -1, args
        assert msg in L.gsvc_last_error(), (args, L.gsvc_last_error())


def test_python_side_refuses_cpu_tensors_and_bad_shapes():
    fmt = FrameFormat("yuv420p")
    a = torch.zeros((1, frame_bytes(4, 4, fmt)), dtype=torch.uint8)
    with pytest.raises(_lib.GsvcError):
        metrics.picture_hash(a, 4, 4, fmt)
    with pytest.raises(ValueError):
        metrics.picture_hash(np.zeros((1, 24), np.uint8), 4, 4, fmt)
    with pytest.raises(ValueError):
        metrics.picture_hash(a, 3, 4, fmt)
