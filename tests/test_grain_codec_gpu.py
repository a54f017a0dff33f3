"""GPU tests of film grain through the codec, built like tests/test_sequence_gpu.py: a 16-frame 64 x 48 yuv420p clip
with KNOWN synthetic noise (the reference grain of tests/_grain_ref.py on ``SyntheticFrameCube(48, 64, 16, seed=7)``) is encoded as two
groups of pictures with ``film_grain=True`` (two tiny fits) and written as one sequence file.  The file carries GRAN; the decoder
verifies every frame with grain on (PHSH is the hash of the UNGRAINED picture); the grained frames are the reference's grain on the
ungrained ones, bit for bit, under each frame's index in the whole clip; grain off equals the file stripped of GRAN; a range of frames
across the cut equals the same frames of the full decode; a file encoded without the flag has no GRAN.

The fits are 40 steps long: their pictures are far from the source, so the two rejection thresholds of the statistics are opened
(``grain_max_residual=255``, ``grain_flat_threshold=65535``) and every whole block counts — what is tested here is the path of the
parameters through the codec, not what a good fit would estimate."""
import os
import sys

import numpy as np
import pytest
import torch

from gsvc_amd import bitstream as B
from gsvc_amd import sequence as S
from gsvc_amd.frames_out import FrameFormat, Y4MWriter, frame_bytes, read_y4m
from tests import _grain_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, T, GOP = 48, 64, 16, 8
FMT = FrameFormat("yuv420p")
NB = frame_bytes(H, W, FMT)
FIT = dict(steps=40, anchors=2000, slab_frames=8.0, densify_grad_threshold=2e-5)
OPEN = dict(grain_max_residual=255, grain_flat_threshold=65535)
sys.path.insert(0, os.path.join(ROOT, "tools"))


class _Keep:
    """A sink that keeps its frames."""

    def __init__(self):
        self.rows, self.bytes = [], 0

    def write(self, frame_u8):
        self.rows.append(np.array(frame_u8, copy=True))

    def close(self):
        pass


def _decode(what, **kw):
    sink = _Keep()
    fn = S.decode_sequence if isinstance(what, str) else B.decode_video
    res = fn(what, sink, **kw)
    return np.stack(sink.rows), res


def _grained(frames, p, ids):
    return ref.apply_ref(frames, H, W, "yuv420p", 8, "limited", p.seed, p.scale, p.kx, p.ky, ids)


@pytest.fixture(scope="module")
def coded(tmp_path_factory):
    """{"clip": the noisy Y4M file, "file": the .gsvs of two GOPs with grain, "gops": their file images, "logs", "tmp"}."""
    from gsvc_amd.fit_setup import encode_gop
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import frames_to_u8
    tmp = tmp_path_factory.mktemp("grain")
    dev = torch.device("cuda", 0)
    cube = SyntheticFrameCube(H, W, T, seed=7, device="cuda")
    clean = frames_to_u8([cube._image(t) for t in range(T)], FMT).cpu().numpy().copy()
    del cube
    noisy = ref.apply_ref(clean, H, W, "yuv420p", 8, "limited", 99, [[1200] * 17, [800] * 17, [800] * 17], [12, 0, 0], [8, 0, 0], list(range(T)))
    assert not np.array_equal(noisy, clean)
    clip = str(tmp / "noisy.y4m")
    with Y4MWriter(clip, W, H, (25, 1), FMT) as sink:
        for fr in noisy:
            sink.write(torch.from_numpy(fr))
    gops, logs = [], []
    for first in (0, GOP):
        blob, log = encode_gop(clip, dev, frame_range=(first, first + GOP), film_grain=True, grain_seed=5 + first, **OPEN, **FIT)
        gops.append(blob)
        logs.append(log)
    path = str(tmp / "clip.gsvs")
    S.write_sequence(path, gops, W, H, (25, 1))
    return {"clip": clip, "file": path, "gops": gops, "logs": logs, "tmp": tmp}


def test_the_file_carries_gran_and_the_log_says_what_was_fitted(coded):
    ch, cw = H // 2, W // 2
    for k, (blob, log) in enumerate(zip(coded["gops"], coded["logs"])):
        bs = B.parse_bitstream(blob)
        assert bs.grain is not None and bs.section_bytes["GRAN"] == 122 and bs.hashes is not None and bs.hashes.shape == (GOP, 3)
        assert [t for t, _ in B.unpack_sections(blob)][-2:] == [b"PHSH", b"GRAN"] and log["sections"]["GRAN"] == 122
        assert bs.grain.seed == 5 + GOP * k and bs.grain.source == FrameFormat("yuv420p", rounding="nearest") and not bs.grain.is_zero
        g = log["grain"]
        print("grain log:", g)
        assert g["blocks"] == [GOP * (H // 8) * (W // 8), GOP * (ch // 8) * (cw // 8), GOP * (ch // 8) * (cw // 8)]          # every whole block
        assert g["scale"] == [list(r) for r in bs.grain.scale] and g["kx"] == list(bs.grain.kx) and g["ky"] == list(bs.grain.ky)
        assert g["seed"] == bs.grain.seed and g["source"] == "yuv420p" and g["gain"] == 1.0


def test_grain_is_synthesised_behind_the_hashes_and_is_the_reference(coded):
    blob = coded["gops"][0]
    bs = B.parse_bitstream(blob)
    on, res_on = _decode(bs, fmt=FMT, strict=True)
    assert res_on["film_grain"] is True and res_on["verified"] and res_on["frames_verified"] == GOP and res_on["frames_mismatched"] == 0
    off, res_off = _decode(B.parse_bitstream(blob), fmt=FMT, strict=True, film_grain=False)
    assert res_off["film_grain"] is False and res_off["frames_verified"] == GOP and np.array_equal(res_on["hashes"], res_off["hashes"])
    assert on.shape == off.shape == (GOP, NB) and not np.array_equal(on, off)
    assert np.array_equal(on, _grained(off, bs.grain, list(range(GOP))))                      # a deterministic post-process of the picture
    stripped, res_s = _decode(B.parse_bitstream(B.with_grain(blob, None)), fmt=FMT, strict=True)
    assert res_s["film_grain"] is False and np.array_equal(stripped, off)
    # a batch that does not divide the GOP: the grain of a frame is that of its index, whatever batch it travels in
    on3 = _decode(B.parse_bitstream(blob), fmt=FMT, batch=3, verify=False)[0]
    off3 = _decode(B.parse_bitstream(blob), fmt=FMT, batch=3, verify=False, film_grain=False)[0]
    assert np.array_equal(on3, _grained(off3, bs.grain, list(range(GOP))))
    # device-side frames: the same bytes, and the hook sees the ungrained pictures
    from gsvc_amd.frames_out import render_frames_u8
    pc, cams, pipe, bg = B.parse_bitstream(blob).build_model("cuda")
    with torch.no_grad():
        plain = torch.stack(list(render_frames_u8(cams, pc, pipe, bg, fmt=FMT, batch=8, to_host=False))).cpu().numpy()
        seen = []
        dev = torch.stack(list(render_frames_u8(cams, pc, pipe, bg, fmt=FMT, batch=8, to_host=False, grain=bs.grain,
                                                on_device_batch=lambda rows: seen.append(rows.clone())))).cpu().numpy()
        with pytest.raises(ValueError, match="rgb24"):
            next(render_frames_u8(cams, pc, pipe, bg, fmt=FrameFormat("rgb24"), grain=bs.grain))
    assert np.array_equal(plain, off) and np.array_equal(dev, on) and np.array_equal(torch.cat(seen).cpu().numpy(), off)
    # an rgb24 decode delivers the pictures as they are
    rgb_on, res_rgb = _decode(B.parse_bitstream(blob), fmt=FrameFormat("rgb24"), verify=False)
    assert res_rgb["film_grain"] is False and np.array_equal(rgb_on, _decode(B.parse_bitstream(blob), fmt=FrameFormat("rgb24"), verify=False, film_grain=False)[0])


def test_decoded_batches_are_the_render_batches_and_the_pairing_counts_frames(coded):
    """``fit_setup.decoded_batches`` (what the encoder's three measures decode through) on the first GOP with a batch that does not divide
    it: the batches start at 0, 3, 6, the last one is the short one, and their rows are the frames of ``render_frames_u8`` at that
    batch, byte for byte; ``decoded_against`` pairs them with the source's rows and refuses a source of another length at the end."""
    from gsvc_amd.fit_setup import decoded_against, decoded_batches
    from gsvc_amd.frames_out import render_frames_u8
    dev = torch.device("cuda", 0)
    blob = coded["gops"][0]
    got = list(decoded_batches(B.parse_bitstream(blob), FMT, dev, batch=3))
    assert [first for first, _ in got] == [0, 3, 6] and [tuple(rows.shape) for _, rows in got] == [(3, NB), (3, NB), (2, NB)]
    assert all(rows.dtype == torch.uint8 and rows.device.type == "cuda" for _, rows in got) and torch.is_grad_enabled()
    pc, cams, pipe, bg = B.parse_bitstream(blob).build_model(dev)
    with torch.no_grad():
        want = torch.stack(list(render_frames_u8(cams, pc, pipe, bg, fmt=FMT, batch=3, to_host=False)))
    assert torch.equal(torch.cat([rows for _, rows in got]), want)
    source = read_y4m(coded["clip"])[1][:GOP]
    pairs = list(decoded_against(B.parse_bitstream(blob), source, FMT, dev, "test", batch=3))
    assert torch.equal(torch.cat([rows for rows, _ in pairs]), want) and np.array_equal(torch.cat([src for _, src in pairs]).cpu().numpy(), source)
    with pytest.raises(ValueError, match=f"test: the file decodes to {GOP} frames, the source has {GOP - 1}"):
        list(decoded_against(B.parse_bitstream(blob), source[:GOP - 1], FMT, dev, "test", batch=3))


def test_a_frame_range_across_the_cut_has_the_bytes_of_the_full_decode(coded, capsys):
    import gsvc_decode
    whole, res = _decode(coded["file"], strict=True)
    assert res["film_grain"] is True and res["frames_verified"] == T and [g["film_grain"] for g in res["gops"]] == [True, True]
    off, res_off = _decode(coded["file"], strict=True, film_grain=False)
    assert res_off["film_grain"] is False and not np.array_equal(whole, off)
    # every frame carries the grain of ITS GOP's parameters under its index in the whole clip
    for k in range(2):
        p = B.parse_bitstream(coded["gops"][k]).grain
        ids = list(range(GOP * k, GOP * k + GOP))
        assert np.array_equal(whole[ids], _grained(off[ids], p, ids))
    part, res_p = _decode(coded["file"], frames=(6, 11), strict=True)
    assert [(g["gop"], g["decoded"]) for g in res_p["gops"]] == [(0, 2), (1, 3)] and np.array_equal(part, whole[6:11])
    small = _decode(coded["file"], frames=(10, 13), batch=2, verify=False)[0]                 # (other render batches: other last bits)
    small_off = _decode(coded["file"], frames=(10, 13), batch=2, verify=False, film_grain=False)[0]
    assert np.array_equal(small, _grained(small_off, B.parse_bitstream(coded["gops"][1]).grain, [10, 11, 12]))
    # the tool: grain by default, --no-film-grain without
    out = str(coded["tmp"] / "out.y4m")
    capsys.readouterr()
    assert gsvc_decode.main([coded["file"], "-o", out, "--strict", "--frames", "6:11"]) == 0
    assert '"film_grain": true' in capsys.readouterr().out and np.array_equal(read_y4m(out)[1], whole[6:11])
    assert gsvc_decode.main([coded["file"], "-o", out, "--strict", "--no-film-grain"]) == 0
    assert '"film_grain": false' in capsys.readouterr().out and np.array_equal(read_y4m(out)[1], off)


def test_without_the_flag_the_file_has_no_gran(coded):
    from gsvc_amd.fit_setup import encode_gop
    blob, log = encode_gop(coded["clip"], torch.device("cuda", 0), frame_range=(0, GOP), **FIT)
    assert "grain" not in log and set(log["sections"]) == {"HEAD", "MLPS", "ANCH", "MASK", "HASH", "SLAB", "PHSH"}
    bs = B.parse_bitstream(blob)
    assert bs.grain is None and b"GRAN" not in [t for t, _ in B.unpack_sections(blob)]
    on, res = _decode(bs, fmt=FMT, strict=True)
    assert res["film_grain"] is False and res["frames_verified"] == GOP
    assert np.array_equal(on, _decode(B.parse_bitstream(blob), fmt=FMT, strict=True, film_grain=False)[0])
    rgb = str(coded["tmp"] / "clip.rgb")
    with open(rgb, "wb") as f:
        f.write(bytes(3 * H * W * 2))
    with pytest.raises(ValueError, match="rgb24"):                                            # refused before the fit starts
        encode_gop(rgb, torch.device("cuda", 0), video_size=(W, H), film_grain=True, **FIT)


def test_fit_tool_measures_grain_for_its_rd_point(tmp_path):
    """tools/fit_synthetic.py --video ... --film-grain at the size of tests/test_fit_tool_gpu.py (an 8-step fit: what its statistics hold
    is not this test's subject): the log has "grain", and the file written carries those parameters."""
    import json

    import fit_synthetic
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import frames_to_u8
    h, w, t = 272, 480, 8
    cube = SyntheticFrameCube(h, w, t, seed=3, device="cuda")
    clip = str(tmp_path / "clip.y4m")
    with Y4MWriter(clip, w, h, (25, 1), FMT) as sink:
        for fr in frames_to_u8([cube._image(k) for k in range(t)], FMT).cpu():
            sink.write(fr)
    del cube
    out, coded_file = tmp_path / "rd.json", str(tmp_path / "rd.gsvc")
    fit_synthetic.main(["--video", clip, "--steps", "8", "--anchors", "8000", "--eval-frames", "4", "--slab-frames", "8", "--payload-tol", "1e9",
                        "--film-grain", "--write-bitstream", coded_file, "--json", str(out)])
    log = json.loads(out.read_text())
    bs = B.read_bitstream(coded_file)
    assert bs.grain is not None and log["bitstream_sections"]["GRAN"] == 122 and log["bitstream_bytes"] == os.path.getsize(coded_file)
    assert log["grain"]["scale"] == [list(r) for r in bs.grain.scale] and log["grain"]["kx"] == list(bs.grain.kx) and log["grain"]["seed"] == bs.grain.seed
    assert len(log["grain"]["blocks"]) == 3 and all(0 <= b <= t * (h // 8) * (w // 8) for b in log["grain"]["blocks"])
    res = B.decode_video(bs, B.NullSink(), fmt=FMT, verify=False)
    assert res["frames"] == t and res["film_grain"] is True
