"""GPU tests of reduced-resolution coding through the encoder and the decoder, at the size and fit of
tests/test_tfilter_codec_gpu.py: an 8-frame 96 x 64 yuv420p clip.  ``encode_gop(coded_size=(48, 32))`` fits the resampled source, the
file carries the coded size in HEAD and the display size in DISP, its hashes are those of the coded-size pictures, and the decoder
delivers ``resample_frames`` of them; ``size=`` gives a preview of any file; ``coded_size=None`` leaves log and sections as they were;
the tools carry the options through.

The fits are 40 steps long: what is tested is the path of the frames, not what a fit gains."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from gsvc_amd import bitstream as B
from gsvc_amd import resample as R
from gsvc_amd import sequence as S
from gsvc_amd.frames_out import FrameFormat, Y4MWriter, frame_bytes, read_y4m

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, T = 64, 96, 8
CW, CH = 48, 32
FMT = FrameFormat("yuv420p")
NB, CNB = frame_bytes(H, W, FMT), frame_bytes(CH, CW, FMT)
FIT = dict(steps=40, anchors=2000, slab_frames=8.0, densify_grad_threshold=2e-5)
FIT_ARGS = ["--steps", "40", "--anchors", "2000", "--slab-frames", "8", "--densify-grad-threshold", "2e-5"]
OLD_LOG = {"W", "H", "frames", "steps", "init", "anchors_initial", "loss_domain", "loss_matrix", "distortion", "anchors_coded", "fit_seconds",
           "hash_format", "verify_decode_fps", "sections"}
OLD_SECTIONS = {"HEAD", "MLPS", "ANCH", "MASK", "HASH", "SLAB", "PHSH"}
sys.path.insert(0, os.path.join(ROOT, "tools"))


class Collect:
    """A sink that keeps its frames."""

    def __init__(self):
        self.rows = []

    def write(self, frame_u8):
        self.rows.append(np.array(frame_u8, copy=True).reshape(-1))

    def close(self):
        pass

    def array(self):
        return np.stack(self.rows)


def resampled(frames, H0, W0, H1, W1):
    return R.resample_frames(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), H0, W0, FMT, H1, W1).cpu().numpy()


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """{"path": a Y4M file, "frames": its frames uint8 [8, NB], "tmp"}."""
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import frames_to_u8
    tmp = tmp_path_factory.mktemp("resample")
    cube = SyntheticFrameCube(H, W, T, seed=7, device="cuda")
    clean = frames_to_u8([cube._image(t) for t in range(T)], FMT).cpu().numpy().copy()
    del cube
    noisy = np.clip(np.rint(clean + np.random.default_rng(3).normal(0.0, 2.0, clean.shape)), 0, 255).astype(np.uint8)
    path = str(tmp / "clip.y4m")
    with Y4MWriter(path, W, H, (25, 1), FMT) as sink:
        for fr in noisy:
            sink.write(torch.from_numpy(fr))
    return {"path": path, "frames": noisy, "tmp": tmp}


@pytest.fixture
def handed(monkeypatch):
    """What every ``VideoFileCube`` built while the test runs was given: a list of (frames, frame_size, (width, height) of the cube)."""
    from gsvc_amd import frames_in
    seen = []

    class Recording(frames_in.VideoFileCube):
        def __init__(self, *a, frames=None, frame_size=None, **kw):
            super().__init__(*a, frames=frames, frame_size=frame_size, **kw)
            seen.append((None if frames is None else np.array(frames, copy=True), frame_size, (self.width, self.height, self.scale, self.x_min, self.y_min)))

    monkeypatch.setattr(frames_in, "VideoFileCube", Recording)
    return seen


def test_encode_at_a_coded_size_and_decode_at_the_display_size(clip, handed):
    from gsvc_amd.fit_setup import encode_gop
    dev = torch.device("cuda", 0)
    blob, log = encode_gop(clip["path"], dev, coded_size=(CW, CH), **FIT)
    # the fit was handed exactly resample_frames(source), and its cube has the geometry of the coded size
    want = resampled(clip["frames"], H, W, CH, CW)
    assert len(handed) == 1 and np.array_equal(handed[0][0], want) and handed[0][1] == (CW, CH)
    assert handed[0][2] == (CW, CH, CW / 2, -1.0, -CH / 2 / (CW / 2))
    # the file: HEAD holds the coded size, DISP the display size; the log says both
    bs = B.parse_bitstream(blob)
    assert (bs.header["W"], bs.header["H"], bs.header["frames"]) == (CW, CH, T) and bs.display == (W, H) and bs.display_size == (W, H)
    assert set(log["sections"]) == OLD_SECTIONS | {"DISP"} and list(log["sections"])[-1] == "DISP"
    assert set(log) == OLD_LOG | {"display"} and (log["W"], log["H"]) == (CW, CH)
    assert set(log["display"]) == {"W", "H", "filter", "psnr_y", "psnr_611"} and log["display"]["filter"] == "lanczos3"
    assert (log["display"]["W"], log["display"]["H"]) == (W, H)
    print("display:", log["display"])
    assert 10.0 < log["display"]["psnr_y"] < 60.0 and 10.0 < log["display"]["psnr_611"] < 60.0
    # both decodes pass strict with the file's hashes; the default one delivers resample_frames of the coded one
    coded, shown = Collect(), Collect()
    res_c = B.decode_video(bs, coded, fmt=FMT, strict=True, size="coded")
    res_d = B.decode_video(B.parse_bitstream(blob), shown, fmt=FMT, strict=True)
    for res, size, flag in ((res_c, (CW, CH), False), (res_d, (W, H), True)):
        assert res["verified"] and res["frames_verified"] == T and (res["W"], res["H"]) == size and res["resampled"] is flag
        assert np.array_equal(res["hashes"], bs.hashes)
    assert coded.array().shape == (T, CNB) and shown.array().shape == (T, NB)
    assert np.array_equal(shown.array(), resampled(coded.array(), CH, CW, H, W))
    # the display PSNR of the log is that of these frames against the source
    sse = ((shown.array()[:, :H * W].astype(np.int64) - clip["frames"][:, :H * W].astype(np.int64)) ** 2).sum()
    assert abs(log["display"]["psnr_y"] - 10.0 * np.log10(255.0 ** 2 * T * H * W / sse)) < 1e-9
    # any other size, and an rgb24 decode, which delivers the coded pictures and says so
    small = Collect()
    res = B.decode_video(B.parse_bitstream(blob), small, fmt=FMT, strict=True, size=(24, 16))
    assert (res["W"], res["H"], res["resampled"]) == (24, 16, True) and np.array_equal(small.array(), resampled(coded.array(), CH, CW, 16, 24))
    res = B.decode_video(B.parse_bitstream(blob), B.NullSink(), fmt=FrameFormat("rgb24"))
    assert (res["W"], res["H"], res["resampled"]) == (CW, CH, False)
    with pytest.raises(ValueError, match="ratio"):
        B.decode_video(B.parse_bitstream(blob), B.NullSink(), fmt=FMT, size=(CW * 4 + 2, CH))
    # a sequence of one GOP: the plain file opened as one
    path = str(clip["tmp"] / "one.gsvc")
    with open(path, "wb") as f:
        f.write(blob)
    seq = S.open_sequence(path)
    assert (seq.W, seq.H) == (CW, CH) and seq.display == (W, H) and seq.display_size == (W, H)
    again = Collect()
    res = S.decode_sequence(seq, again, fmt=FMT, strict=True)
    assert (res["W"], res["H"], res["resampled"]) == (W, H, True) and np.array_equal(again.array(), shown.array())
    # what the encoder's display measure decodes through: the render batches of render_frames_u8 at the display size, byte for byte
    from gsvc_amd.fit_setup import decoded_batches
    from gsvc_amd.frames_out import render_frames_u8
    got = list(decoded_batches(B.parse_bitstream(blob), FMT, dev, batch=3, out_size=(H, W)))
    assert [first for first, _ in got] == [0, 3, 6] and [tuple(rows.shape) for _, rows in got] == [(3, NB), (3, NB), (2, NB)]
    pc, cams, pipe, bg = B.parse_bitstream(blob).build_model(dev)
    with torch.no_grad():
        want = torch.stack(list(render_frames_u8(cams, pc, pipe, bg, fmt=FMT, batch=3, to_host=False, out_size=(H, W))))
    assert torch.equal(torch.cat([rows for _, rows in got]), want)


def test_with_denoise_the_fit_is_handed_the_resampled_filtered_frames(clip, handed):
    from gsvc_amd.fit_setup import encode_gop
    from gsvc_amd.tfilter import denoise_frames
    dev = torch.device("cuda", 0)
    blob, log = encode_gop(clip["path"], dev, frame_range=(0, 4), coded_size=(CW, CH), denoise=2.0, **FIT)
    filtered, flog = denoise_frames(torch.from_numpy(np.ascontiguousarray(clip["frames"][:4])).cuda(), H, W, FMT, sigma=2.0)
    want = R.resample_frames(filtered, H, W, FMT, CH, CW).cpu().numpy()
    assert len(handed) == 1 and np.array_equal(handed[0][0], want) and not np.array_equal(want, resampled(clip["frames"][:4], H, W, CH, CW))
    assert log["denoise"] == flog and "display" in log and log["frames"] == 4
    assert B.decode_video(B.parse_bitstream(blob), B.NullSink(), fmt=FMT, strict=True)["frames_verified"] == 4


def test_without_coded_size_nothing_changes_and_any_file_has_a_preview(clip, handed):
    from gsvc_amd.fit_setup import encode_gop
    dev = torch.device("cuda", 0)
    blob, log = encode_gop(clip["path"], dev, **FIT)
    assert len(handed) == 1 and handed[0][0] is None and handed[0][1] is None and handed[0][2][:2] == (W, H)
    assert set(log) == OLD_LOG and set(log["sections"]) == OLD_SECTIONS and (log["W"], log["H"]) == (W, H)
    bs = B.parse_bitstream(blob)
    assert bs.display is None and bs.display_size == (W, H)
    full, small = Collect(), Collect()
    res = B.decode_video(bs, full, fmt=FMT, strict=True)
    assert (res["W"], res["H"], res["resampled"]) == (W, H, False) and full.array().shape == (T, NB)
    res = B.decode_video(B.parse_bitstream(blob), small, fmt=FMT, strict=True, size=(CW, CH))
    assert (res["W"], res["H"], res["resampled"]) == (CW, CH, True) and res["frames_verified"] == T
    assert np.array_equal(small.array(), resampled(full.array(), H, W, CH, CW))
    same = Collect()
    assert B.decode_video(B.parse_bitstream(blob), same, fmt=FMT, size="coded")["resampled"] is False and np.array_equal(same.array(), full.array())


def test_refusals_before_anything_is_fitted(clip, handed, tmp_path):
    from gsvc_amd.fit_setup import encode_gop
    dev = torch.device("cuda", 0)
    flows = tmp_path / "flows"
    flows.mkdir()
    rgb = str(tmp_path / "clip.rgb")
    with open(rgb, "wb") as f:
        f.write(bytes(3 * H * W * 2))
    for kw, what in ((dict(coded_size=(CW, CH), film_grain=True), "film_grain"), (dict(coded_size=(CW, CH), flow_dir=str(flows)), "flow_dir"),
                     (dict(coded_size=(W // 4 - 2, CH)), "ratio"), (dict(coded_size=(CW, H * 4 + 2)), "ratio"), (dict(coded_size=(CW + 1, CH)), "even"),
                     (dict(coded_size=(CW, CH - 1)), "even"), (dict(coded_size=(CW,)), "coded_size"), (dict(coded_size=(CW, CH), frame_range=(4, 4)), "frame_range")):
        with pytest.raises(ValueError, match=what):
            encode_gop(clip["path"], dev, **kw, **FIT)
    with pytest.raises(ValueError, match="rgb24"):
        encode_gop(rgb, dev, video_size=(W, H), coded_size=(CW, CH), **FIT)
    assert handed == []                                                        # no cube was built, nothing was fitted
    from gsvc_amd.frames_in import VideoFileCube
    with pytest.raises(ValueError, match="frame_size"):
        VideoFileCube(clip["path"], device=dev, frame_size=(CW, CH))
    with pytest.raises(ValueError, match="frames must be"):
        VideoFileCube(clip["path"], device=dev, frames=clip["frames"], frame_size=(CW, CH))
    from gsvc_amd.frames_out import render_frames_u8
    with pytest.raises(ValueError, match="rgb24"):
        next(render_frames_u8([object()], None, None, None, fmt=FrameFormat("rgb24"), out_size=(H, W)))


def test_the_tools_carry_the_sizes_through(clip, capsys, handed):
    import gsvc_decode
    import gsvc_encode
    import scale_video
    coded = str(clip["tmp"] / "clip.gsvs")
    log = gsvc_encode.main([clip["path"], "-o", coded, "--gop-frames", "4", "--min-gop", "2", "--coded-size", f"{CW}x{CH}"] + FIT_ARGS)
    assert [(g["first"], g["frames"]) for g in log["gops"]] == [(0, 4), (4, 4)] and (log["W"], log["H"]) == (CW, CH)
    assert log["display"] == {"W": W, "H": H, "filter": "lanczos3"} and all(g["display"]["W"] == W and "DISP" in g["sections"] for g in log["gops"])
    assert log["bpp"] == 8.0 * log["total_bytes"] / (H * W * T)                 # over display pixels
    want = resampled(clip["frames"], H, W, CH, CW)
    assert len(handed) == 2 and np.array_equal(handed[0][0], want[:4]) and np.array_equal(handed[1][0], want[4:])
    seq = S.open_sequence(coded)
    assert (seq.W, seq.H) == (CW, CH) and seq.display_size == (W, H) and [seq.gop(k).display for k in range(2)] == [(W, H)] * 2
    shown, small = str(clip["tmp"] / "shown.y4m"), str(clip["tmp"] / "small.y4m")
    capsys.readouterr()
    assert gsvc_decode.main([coded, "-o", shown, "--strict"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (line["W"], line["H"], line["resampled"], line["frames_verified"]) == (W, H, True, T)
    assert gsvc_decode.main([coded, "-o", small, "--strict", "--size", "coded"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (line["W"], line["H"], line["resampled"], line["frames_verified"]) == (CW, CH, False, T)
    hdr_d, got_d = read_y4m(shown)
    hdr_c, got_c = read_y4m(small)
    assert (hdr_d["W"], hdr_d["H"], hdr_d["fps"]) == (W, H, (25, 1)) and got_d.shape == (T, NB)
    assert (hdr_c["W"], hdr_c["H"]) == (CW, CH) and got_c.shape == (T, CNB)
    assert np.array_equal(got_d, resampled(got_c, CH, CW, H, W))
    # GOPs that disagree about DISP are refused
    blobs = [seq.gop_image(0), B.with_display(seq.gop_image(1), (W, H + 2))]
    mixed = str(clip["tmp"] / "mixed.gsvs")
    S.write_sequence(mixed, blobs, CW, CH, (25, 1))
    with pytest.raises(B.BitstreamError, match="DISP"):
        S.decode_sequence(mixed, B.NullSink(), fmt=FMT)
    # the scaler writes what resample_frames returns
    out = str(clip["tmp"] / "scaled.y4m")
    slog = scale_video.main([clip["path"], out, "--size", "144x40"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["frames"] == T
    hdr, got = read_y4m(out)
    assert (hdr["W"], hdr["H"], hdr["fps"], hdr["layout"], hdr["depth"]) == (144, 40, (25, 1), "yuv420p", 8)
    assert np.array_equal(got, resampled(clip["frames"], H, W, 40, 144))
    assert (slog["W"], slog["H"], slog["source_W"], slog["source_H"], slog["frames"], slog["format"]) == (144, 40, W, H, T, "yuv420p")
