"""CPU tests of the group-of-pictures layer: the GOP plan (gsvc_amd/scene.py, ``plan_gops``) on the cases that can
go wrong and as properties over a seeded sweep, the histogram distance and the cuts on hand-made histograms, the sequence file's framing
(gsvc_amd/sequence.py) on synthetic GOP images built as tests/test_bitstream_cpu.py builds its file, and the argument checks of
``VideoFileCube(frame_range=...)``, ``gsvc_frames_histogram`` and ``metrics.plane_histograms`` that need no device."""
import struct
import zlib

import numpy as np
import pytest
import torch

from gsvc_amd import _lib, bitstream as B, metrics, scene, sequence as S
from gsvc_amd.frames_out import FrameFormat, Y4MWriter, frame_bytes
from gsvc_amd.stream_codec import StreamPack
from tests import _scene_ref as ref


# ---- plan_gops ----------------------------------------------------------------------------------------------------------------------
def _tiles(plan, T):
    at = 0
    for first, count in plan:
        assert first == at and count >= 1
        at += count
    return at == T


def test_plan_without_cuts_splits_evenly_longer_gops_first():
    assert scene.plan_gops(64, [], 32, 4) == [(0, 32), (32, 32)]
    assert scene.plan_gops(65, [], 32, 4) == [(0, 22), (22, 22), (44, 21)]          # a multiple of gop_frames + 1: three GOPs, not 32 + 32 + 1
    assert scene.plan_gops(63, [], 32, 4) == [(0, 32), (32, 31)]                     # a multiple - 1
    assert scene.plan_gops(32, [], 32, 4) == [(0, 32)] and scene.plan_gops(33, [], 32, 4) == [(0, 17), (17, 16)]
    assert scene.plan_gops(16, [], 8, 4) == [(0, 8), (8, 8)]


def test_plan_with_cuts():
    assert scene.plan_gops(16, [8], 12, 4) == [(0, 8), (8, 8)]
    assert scene.plan_gops(40, [10], 16, 4) == [(0, 10), (10, 15), (25, 15)]
    # cuts closer together than min_gop: the short scene joins the one before it
    assert scene.plan_gops(40, [10, 12], 32, 4) == [(0, 12), (12, 28)]
    assert scene.plan_gops(40, [10, 12, 13, 14], 32, 4) == [(0, 14), (14, 26)]
    # a first scene that is too short joins the next
    assert scene.plan_gops(40, [2], 32, 4) == [(0, 20), (20, 20)] == scene.plan_gops(40, [], 32, 4)
    assert scene.plan_gops(40, [2, 6], 32, 4) == [(0, 6), (6, 17), (23, 17)]          # (2 + 4 frames: long enough, the scene is closed)
    assert scene.plan_gops(40, [2, 20], 32, 4) == [(0, 20), (20, 20)]
    assert scene.plan_gops(40, [2, 3, 20], 32, 4) == [(0, 20), (20, 20)]
    # a last scene that is too short joins the previous
    assert scene.plan_gops(40, [38], 64, 4) == [(0, 40)]
    # cuts outside (0, T), unsorted and repeated
    assert scene.plan_gops(40, [20, 0, 40, 99, -3, 20], 32, 4) == [(0, 20), (20, 20)]


def test_plan_of_a_clip_shorter_than_min_gop_is_one_gop():
    assert scene.plan_gops(3, [], 8, 4) == [(0, 3)] and scene.plan_gops(3, [1, 2], 8, 4) == [(0, 3)] and scene.plan_gops(1, [], 8, 4) == [(0, 1)]


def test_plan_refusals():
    with pytest.raises(ValueError, match="2 x min_gop"):
        scene.plan_gops(64, [], 7, 4)
    with pytest.raises(ValueError, match="min_gop"):
        scene.plan_gops(64, [], 8, 1)
    with pytest.raises(ValueError):
        scene.plan_gops(0, [], 8, 4)


def test_plan_properties_over_a_seeded_sweep():
    rng = np.random.default_rng(5)
    for _ in range(400):
        min_gop = int(rng.integers(2, 9))
        gop_frames = int(rng.integers(2 * min_gop, 2 * min_gop + 40))
        T = int(rng.integers(1, 400))
        cuts = sorted(set(rng.integers(0, T + 2, int(rng.integers(0, 12))).tolist()))
        plan = scene.plan_gops(T, cuts, gop_frames, min_gop)
        assert _tiles(plan, T), (T, cuts, gop_frames, min_gop, plan)
        assert plan == scene.plan_gops(T, list(reversed(cuts)), gop_frames, min_gop)
        if T < min_gop:
            assert plan == [(0, T)]
        else:
            assert all(min_gop <= c <= gop_frames for _, c in plan), (T, cuts, gop_frames, min_gop, plan)
        # a GOP boundary that is not a cut lies inside a scene; a cut between two scenes of min_gop frames or more is a boundary
        starts = [0] + [c for c in cuts if 0 < c < T] + [T]
        firsts = {f for f, _ in plan}
        for a, c, b in zip(starts, starts[1:], starts[2:]):
            if c - a >= min_gop and b - c >= min_gop and all(y - x >= min_gop for x, y in zip(starts, starts[1:])):
                assert c in firsts
        assert scene.gop_cut_flags(plan, cuts) == [1 if f in cuts and f > 0 else 0 for f, _ in plan]


# ---- the distance and the cuts --------------------------------------------------------------------------------------------------------
def _hist_of(codes_per_frame):
    h = np.zeros((len(codes_per_frame), 3, 256), np.int64)
    for t, codes in enumerate(codes_per_frame):
        h[t, 0] = np.bincount(np.asarray(codes), minlength=256)
        h[t, 1, 128] = h[t, 2, 128] = len(codes) // 4
    return h


def test_distance_on_hand_made_histograms():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, 96)
    # a permutation of the same pixels: 0;  disjoint code ranges: exactly 1
    h = _hist_of([a, rng.permutation(a), np.arange(96) % 64, 64 + np.arange(96) % 64])
    d = scene.histogram_distance(h)
    assert d.dtype == np.float64 and d.shape == (3,) and d[0] == 0.0 and d[2] == 1.0 and 0.0 < d[1] <= 1.0
    assert d.tolist() == ref.distance_ref(h) and scene.histogram_distance(h, bins=256).tolist() == ref.distance_ref(h, bins=256)
    # by hand: 4 samples, one moves from code 10 to code 200 -> |-1| + |+1| over 2 * 4
    h2 = _hist_of([[10, 10, 50, 50], [10, 200, 50, 50]])
    assert scene.histogram_distance(h2).tolist() == [0.25]
    # folding to 64 bins: codes 8 and 11 share bin 2 (distance 0), codes 11 and 12 do not (1); at 256 bins both pairs differ
    h3 = _hist_of([[8] * 4, [11] * 4, [12] * 4])
    assert scene.histogram_distance(h3, bins=64).tolist() == [0.0, 1.0] and scene.histogram_distance(h3, bins=256).tolist() == [1.0, 1.0]
    # rgb24 reads channel 1; luma rows are taken as they are
    assert scene.histogram_distance(h3, layout="rgb24").tolist() == [0.0, 0.0]
    assert scene.histogram_distance(h3[:, 0]).tolist() == [0.0, 1.0]
    assert scene.histogram_distance(h3[:1]).shape == (0,)
    with pytest.raises(ValueError, match="same"):
        scene.histogram_distance(_hist_of([[1, 2, 3], [1, 2]]))
    with pytest.raises(ValueError, match="fold"):
        scene.histogram_distance(h3, bins=48)


def test_cuts_from_distances():
    d = [0.1, 0.9, 0.2, 0.6, 0.7, 0.0]
    assert scene.scene_cuts(d) == [2, 4, 5] and scene.scene_cuts(d, threshold=0.65) == [2, 5] and scene.scene_cuts(d, threshold=0.95) == []
    assert scene.scene_cuts(d, min_gop=2) == [2, 4] and scene.scene_cuts(d, min_gop=3) == [4]
    assert scene.scene_cuts([0.5]) == [] and scene.scene_cuts([]) == []          # strictly above the threshold


# ---- the sequence file on synthetic GOP images ----------------------------------------------------------------------------------------
class _Shape:
    """What ``make_header`` reads of a model (as in tests/test_bitstream_cpu.py)."""
    feat_dim, n_offsets, voxel_size, update_depth, update_init_factor, update_hierachy_factor = 50, 10, 0.001, 3, 16, 4
    n_features_per_level, log2_hashmap_size, log2_hashmap_size_2D = 8, 13, 15
    resolutions_list, resolutions_list_2D = (18, 24, 33, 44), (130, 258)
    use_2D, ste_binary, ste_multistep, add_noise, Q = True, True, False, False, 1
    x_bound_min, x_bound_max = torch.tensor([[-1.1, -0.825, -0.1375]]), torch.tensor([[1.1, 0.825, 0.1375]])

    class model_config:
        time_multi_res, offset_multi_res = 16, 16


def _gop(seed, frames=8, W=64, fps=(30000, 1001)):
    rng = np.random.default_rng(seed)
    pack = StreamPack(n_full=1200, n=1000, anchor_interval=np.array([3e-5, 2e-5, 1e-5], np.float32), anchor_min=np.array([-1.1, -0.8, -0.1], np.float32),
                      anchors_q=None, prob_masks=float(np.float32(0.37)), prob_hash=float(np.float32(0.501)), slabs=[(0, 400), (400, 1000)],
                      feat=[rng.bytes(300), rng.bytes(211)], scaling=[rng.bytes(90), rng.bytes(77)], offsets=[rng.bytes(120), b""],
                      masks=rng.bytes(64), hash=rng.bytes(500), anchor_stream=rng.bytes(333))
    geo = B.CubeGeometry(W=W, H=48, frames=frames, scale=32.0, x_min=-1.0, y_min=-0.75, z_min=-0.125, threshold=0.125, fps=fps)
    h = rng.integers(0, 2 ** 63, (frames, 3), dtype=np.uint64)
    return B.bitstream_bytes(_Shape, pack, geo, rng.bytes(800), (FrameFormat("yuv420p"), h))


def _gop_at(blob, k):
    """(offset, length) of the k-th GOPU payload of a sequence file's bytes."""
    count = struct.unpack_from("<H", blob, 6)[0]
    at, seen = 8 + 16 * count, -1
    for i in range(count):
        tag, length, _ = struct.unpack_from("<4sQI", blob, 8 + 16 * i)
        if tag == b"GOPU":
            seen += 1
            if seen == k:
                return at, length
        at += length
    raise AssertionError(k)


def test_sequence_round_trip(tmp_path):
    gops = [_gop(1, 8), _gop(2, 5), _gop(3, 8)]
    path = tmp_path / "clip.gsvs"
    written = S.write_sequence(path, gops, 64, 48, (30000, 1001), [0, 1, 0])
    blob = path.read_bytes()
    assert written == {"bytes": len(blob), "gops": 3} and blob[:4] == b"GSVS" and struct.unpack_from("<HH", blob, 4) == (1, 4)
    tag, length, crc = struct.unpack_from("<4sQI", blob, 8 + 16 * 2)
    assert (tag, length, crc) == (b"GOPU", len(gops[1]), zlib.crc32(gops[1]))
    seq = S.open_sequence(path)
    assert (seq.W, seq.H, seq.fps, seq.frames, seq.file_bytes) == (64, 48, (30000, 1001), 21, len(blob))
    assert seq.gops == [(0, 8), (8, 5), (13, 8)] and seq.cuts == [0, 1, 0] and [seq.gop_bytes(k) for k in range(3)] == [len(g) for g in gops]
    g = seq.geometry
    assert (g.W, g.H, g.frames, g.fps) == (64, 48, 21, (30000, 1001))
    for k, image in enumerate(gops):
        bs, alone = seq.gop(k), B.parse_bitstream(image)
        assert bs.header["frames"] == seq.gops[k][1] and bs.file_bytes == len(image) and bs.mlp_bytes == alone.mlp_bytes
        assert np.array_equal(bs.hashes, alone.hashes) and bs.hash_format == FrameFormat("yuv420p", rounding="nearest")
    assert seq.hash_format == FrameFormat("yuv420p", rounding="nearest")
    with pytest.raises(IndexError):
        seq.gop(3)
    # parse_bitstream still refuses the new magic by name
    with pytest.raises(B.BitstreamError) as e:
        B.parse_bitstream(blob)
    assert e.value.section == "magic"
    with pytest.raises(ValueError, match="at least one GOP"):
        S.sequence_bytes([], 64, 48, (30, 1))
    with pytest.raises(ValueError, match="not a bitstream file image"):
        S.sequence_bytes([b"GSVX" + gops[0][4:]], 64, 48, (30, 1))


def test_a_plain_bitstream_file_is_a_sequence_of_one(tmp_path):
    image = _gop(4, 8)
    path = tmp_path / "clip.gsvc"
    path.write_bytes(image)
    seq = S.open_sequence(path)
    assert seq.gops == [(0, 8)] and seq.cuts == [0] and (seq.W, seq.H, seq.frames, seq.fps) == (64, 48, 8, (30000, 1001))
    assert seq.gop(0).mlp_bytes == B.parse_bitstream(image).mlp_bytes and seq.gop_bytes(0) == len(image)
    bad = bytearray(image)
    bad[-1] ^= 0x10                                   # its errors stay its own: the last section is PHSH
    path.write_bytes(bytes(bad))
    with pytest.raises(B.BitstreamError) as e:
        S.open_sequence(path).gop(0)
    assert e.value.section == "PHSH"


def test_damage_is_named_by_gop(tmp_path):
    gops = [_gop(1), _gop(2), _gop(3)]
    blob = S.sequence_bytes(gops, 64, 48, (30000, 1001))
    path = tmp_path / "bad.gsvs"
    at, length = _gop_at(blob, 1)
    for where in (at, at + length // 2, at + length - 1):
        bad = bytearray(blob)
        bad[where] ^= 0x01
        path.write_bytes(bytes(bad))
        seq = S.open_sequence(path)                   # the header is intact: the file opens, GOP 0 and GOP 2 read
        assert seq.gop(0).header["frames"] == 8 and seq.gop(2).header["frames"] == 8
        with pytest.raises(B.BitstreamError, match=r"GOPU\[1\].*CRC") as e:
            seq.gop(1)
        assert e.value.section == "GOPU[1]"
    # a GOP that ends early
    path.write_bytes(blob[:_gop_at(blob, 2)[0] + 100])
    with pytest.raises(B.BitstreamError, match="truncated") as e:
        S.open_sequence(path).gop(2)
    assert e.value.section == "GOPU[2]"
    # damage INSIDE a GOP image under a correct outer CRC: the inner section stays in the message
    inner = bytearray(gops[1])
    inner[-1] ^= 0x01
    path.write_bytes(_raw_sequence(S.pack_fields(_seqh([8, 8, 8])), [gops[0], bytes(inner), gops[2]]))
    with pytest.raises(B.BitstreamError, match=r"GOPU\[1\]: section PHSH: CRC") as e:
        S.open_sequence(path).gop(1)
    assert e.value.section == "GOPU[1]"


def _seqh(counts, W=64, frames=None, firsts=None, fps=(30000, 1001)):
    firsts = [int(v) for v in np.cumsum([0] + counts[:-1])] if firsts is None else firsts
    return {"W": W, "H": 48, "fps_num": fps[0], "fps_den": fps[1], "frames": sum(counts) if frames is None else frames, "gop_first": firsts,
            "gop_frames": counts, "gop_cut": [0] * len(counts)}


def _raw_sequence(seqh: bytes, gops, magic=b"GSVS", version=1):
    sections = [(b"SEQH", seqh)] + [(b"GOPU", g) for g in gops]
    out = [struct.pack("<4sHH", magic, version, len(sections))]
    out += [struct.pack("<4sQI", t, len(p), zlib.crc32(p)) for t, p in sections]
    return b"".join(out + [p for _, p in sections])


def test_truncation_and_a_bad_header(tmp_path):
    gops = [_gop(1), _gop(2)]
    blob = S.sequence_bytes(gops, 64, 48, (30000, 1001))
    assert blob == _raw_sequence(S.pack_fields(_seqh([8, 8])), gops)
    path = tmp_path / "t.gsvs"
    table_end = 8 + 16 * 3
    seqh_len = struct.unpack_from("<4sQI", blob, 8)[1]
    for cut, where in ((0, "magic"), (3, "magic"), (6, "version"), (8, "table"), (table_end - 1, "table"), (table_end, "SEQH"),
                       (table_end + seqh_len - 1, "SEQH")):
        path.write_bytes(blob[:cut])
        with pytest.raises(B.BitstreamError) as e:
            S.open_sequence(path)
        assert e.value.section == where, cut
    bad = bytearray(blob)
    bad[table_end + 5] ^= 0x20
    path.write_bytes(bytes(bad))
    with pytest.raises(B.BitstreamError, match="CRC") as e:
        S.open_sequence(path)
    assert e.value.section == "SEQH"
    for raw, where, text in ((_raw_sequence(S.pack_fields(_seqh([8, 8])), gops, version=2), "version", "version 2"),
                             (_raw_sequence(S.pack_fields(_seqh([8, 8])), gops, magic=b"GSVX"), "magic", "neither"),
                             # an index that leaves a gap, one that overlaps, one that ends early, one GOP too few
                             (_raw_sequence(S.pack_fields(_seqh([8, 8], firsts=[0, 9], frames=17)), gops), "SEQH", "tile"),
                             (_raw_sequence(S.pack_fields(_seqh([8, 8], firsts=[0, 7])), gops), "SEQH", "tile"),
                             (_raw_sequence(S.pack_fields(_seqh([8, 8], frames=20)), gops), "SEQH", "tile"),
                             (_raw_sequence(S.pack_fields(_seqh([8])), gops), "SEQH", "GOPs"),
                             (_raw_sequence(S.pack_fields({k: v for k, v in _seqh([8, 8]).items() if k != "gop_cut"}), gops), "SEQH", "gop_cut")):
        path.write_bytes(raw)
        with pytest.raises(B.BitstreamError, match=text) as e:
            S.open_sequence(path)
        assert e.value.section == where, text


def test_a_gop_that_disagrees_with_the_header_is_refused(tmp_path):
    path = tmp_path / "w.gsvs"
    path.write_bytes(_raw_sequence(S.pack_fields(_seqh([8, 8])), [_gop(1), _gop(2, W=66)]))          # a GOP whose W differs
    seq = S.open_sequence(path)
    assert seq.gop(0).header["W"] == 64
    with pytest.raises(B.BitstreamError, match=r"GOPU\[1\].*W = 66") as e:
        seq.gop(1)
    assert e.value.section == "GOPU[1]"
    path.write_bytes(_raw_sequence(S.pack_fields(_seqh([8, 7])), [_gop(1), _gop(2)]))                # ... whose frame count differs
    with pytest.raises(B.BitstreamError, match=r"GOPU\[1\].*frames = 8"):
        S.open_sequence(path).gop(1)
    path.write_bytes(_raw_sequence(S.pack_fields(_seqh([8, 8], fps=(25, 1))), [_gop(1, fps=(25, 1)), _gop(2, fps=(30, 1))]))          # ... whose rate differs
    with pytest.raises(B.BitstreamError, match=r"GOPU\[1\].*fps_num = 30"):
        S.open_sequence(path).gop(1)


# ---- what is refused before a device is needed ----------------------------------------------------------------------------------------
def test_frame_range_argument_checks(tmp_path):
    from gsvc_amd.frames_in import VideoFileCube
    fmt = FrameFormat("yuv420p")
    clip = str(tmp_path / "clip.y4m")
    with Y4MWriter(clip, 8, 4, (25, 1), fmt) as sink:
        for t in range(6):
            sink.write(np.full(frame_bytes(4, 8, fmt), 16 + t, np.uint8))
    for bad in ((0, 7), (3, 3), (4, 2), (-1, 3), (6, 7), (1,), (1, 2, 3), "ab", 5):
        with pytest.raises(ValueError, match="frame_range"):
            VideoFileCube(clip, device="cpu", frame_range=bad)
    with pytest.raises(_lib.GsvcError, match="CUDA device"):          # a good range gets as far as an unranged cube does without a device
        VideoFileCube(clip, device="cpu", frame_range=(2, 5))
    with pytest.raises(_lib.GsvcError, match="CUDA device"):
        VideoFileCube(clip, device="cpu")


def test_histogram_entry_point_validates_on_the_host():
    L = _lib.lib()
    ok = (64, 48, 1, 4, 4, 0, 8, 256, None)          # frames, stride, n, H, W, layout, depth, out, stream
    cases = [((None,) + ok[1:], b"NULL"), (ok[:7] + (None, None), b"NULL"), (ok[:2] + (0,) + ok[3:], b"n must be"),
             (ok[:2] + (65536,) + ok[3:], b"n must be"), (ok[:5] + (3,) + ok[6:], b"unknown layout"), (ok[:6] + (7,) + ok[7:], b"depth must be"),
             (ok[:6] + (17,) + ok[7:], b"depth must be"), (ok[:6] + (10,) + ok[7:], b"rgb24 frames are 8-bit"),
             ((64, 48, 1, 3, 4, 2, 8, 256, None), b"even"), ((64, 47, 1, 4, 4, 0, 8, 256, None), b"shorter than a frame"),
             ((65, 96, 1, 4, 4, 1, 10, 256, None), b"2-byte aligned"), ((64, 97, 1, 4, 4, 1, 10, 256, None), b"multiple of 2"),
             ((64, 48, 1, 0, 4, 0, 8, 256, None), b"image size"), ((64, 48, 1, 4, 4, 0, 8, 258, None), b"4-byte aligned")]
    for args, msg in cases:
        assert L.gsvc_frames_histogram(*args) == -1, args
        err = L.gsvc_last_error()
        assert msg in err and err.startswith(b"frames_histogram:"), (args, err)


def test_plane_histograms_refuses_cpu_tensors_and_bad_shapes():
    fmt = FrameFormat("yuv420p")
    a = torch.zeros((1, frame_bytes(4, 4, fmt)), dtype=torch.uint8)
    with pytest.raises(_lib.GsvcError, match="CPU tensors are not supported"):
        metrics.plane_histograms(a, 4, 4, fmt)
    with pytest.raises(ValueError):
        metrics.plane_histograms(np.zeros((1, 24), np.uint8), 4, 4, fmt)
    with pytest.raises(ValueError):
        metrics.plane_histograms(a, 3, 4, fmt)
    with pytest.raises(_lib.GsvcError, match="CUDA device"):
        scene.video_histograms(({"H": 4, "W": 4, "fmt": fmt, "frame_bytes": 24}, np.zeros((2, 24), np.uint8)), device="cpu")


def test_reference_histogram_by_hand():
    """A 2 x 2 4:2:0 frame, 8-bit and as 10-bit words: the bin is the code's upper eight bits; stray bits above the depth land in 255."""
    h = ref.histogram_ref(np.array([[7, 7, 255, 16, 128, 64]], np.uint8), 2, 2, "yuv420p", 8)
    assert h.shape == (1, 3, 256) and h[0, 0, 7] == 2 and h[0, 0, 255] == 1 and h[0, 0, 16] == 1 and h[0, 1, 128] == 1 and h[0, 2, 64] == 1
    assert h.sum() == 6
    deep = np.array([[1023, 4, 3, 0xFFFF, 512, 256]], "<u2").view(np.uint8)
    h = ref.histogram_ref(deep, 2, 2, "yuv420p", 10)
    assert h[0, 0, 255] == 2 and h[0, 0, 1] == 1 and h[0, 0, 0] == 1 and h[0, 1, 128] == 1 and h[0, 2, 64] == 1
    rgb = ref.histogram_ref(np.array([[1, 2, 3, 1, 5, 6]], np.uint8), 1, 2, "rgb24", 8)
    assert rgb[0, 0, 1] == 2 and rgb[0, 1, 2] == 1 and rgb[0, 1, 5] == 1 and rgb[0, 2, 3] == 1 and rgb[0, 2, 6] == 1
