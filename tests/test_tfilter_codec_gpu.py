"""GPU tests of the temporal prefilter through the encoder, at the size and fit of tests/test_grain_codec_gpu.py: a
16-frame 64 x 48 yuv420p clip of two different contents (a cut at frame 8) with white noise on its codes.  ``encode_gop(denoise=...)``
fits the filtered frames and says so in its log, the file decodes ``--strict``; with ``film_grain`` the grain statistics are those
against the ORIGINAL source; ``denoise=None`` leaves log and sections as they were; tools/gsvc_encode.py ``--gop-frames 8 --denoise``
filters every GOP on its own; tools/denoise_video.py writes what ``denoise_frames`` returns.

The fits are 40 steps long: what is tested is the path of the frames through the encoder, not what a fit gains."""
import os
import sys

import numpy as np
import pytest
import torch

from gsvc_amd import bitstream as B
from gsvc_amd import sequence as S
from gsvc_amd import tfilter as TF
from gsvc_amd.frames_out import FrameFormat, Y4MWriter, frame_bytes, read_y4m

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, T, GOP = 48, 64, 16, 8
FMT = FrameFormat("yuv420p")
NB = frame_bytes(H, W, FMT)
FIT = dict(steps=40, anchors=2000, slab_frames=8.0, densify_grad_threshold=2e-5)
FIT_ARGS = ["--steps", "40", "--anchors", "2000", "--slab-frames", "8", "--densify-grad-threshold", "2e-5"]
OPEN = dict(grain_max_residual=255, grain_flat_threshold=65535)
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """{"path": the noisy Y4M file, "frames": its frames uint8 [16, NB] (frames 0 .. 7 and 8 .. 15 show different content), "tmp"}."""
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import frames_to_u8
    tmp = tmp_path_factory.mktemp("tfilter")
    parts = []
    for seed in (7, 21):
        cube = SyntheticFrameCube(H, W, GOP, seed=seed, device="cuda")
        parts.append(frames_to_u8([cube._image(t) for t in range(GOP)], FMT).cpu().numpy().copy())
        del cube
    clean = np.concatenate(parts)
    if np.abs(clean[7].astype(int) - clean[8].astype(int)).mean() < 4:          # (the cut must be one)
        clean[GOP:] = 255 - clean[GOP:]
    rng = np.random.default_rng(3)
    noisy = np.clip(np.rint(clean + rng.normal(0.0, 2.5, clean.shape)), 0, 255).astype(np.uint8)
    path = str(tmp / "noisy.y4m")
    with Y4MWriter(path, W, H, (25, 1), FMT) as sink:
        for fr in noisy:
            sink.write(torch.from_numpy(fr))
    return {"path": path, "frames": noisy, "tmp": tmp}


@pytest.fixture
def handed(monkeypatch):
    """The ``frames`` every ``VideoFileCube`` built while the test runs was given (``encode_gop`` builds the cube of its fit): a list."""
    from gsvc_amd import frames_in
    seen = []

    class Recording(frames_in.VideoFileCube):
        def __init__(self, *a, frames=None, **kw):
            seen.append(None if frames is None else np.array(frames, copy=True))
            super().__init__(*a, frames=frames, **kw)

    monkeypatch.setattr(frames_in, "VideoFileCube", Recording)
    return seen


def _filtered(frames, **kw):
    out, log = TF.denoise_frames(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), H, W, FMT, **kw)
    return out.cpu().numpy(), log


def test_encode_gop_fits_the_filtered_frames_and_grain_is_measured_against_the_original(clip, handed):
    from gsvc_amd.fit_setup import encode_gop, grain_statistics
    from gsvc_amd.frames_in import VideoFileCube
    from gsvc_amd.grain import fit_grain
    dev = torch.device("cuda", 0)
    blob, log = encode_gop(clip["path"], dev, frame_range=(0, GOP), denoise="auto", film_grain=True, grain_seed=5, **OPEN, **FIT)
    want, want_log = _filtered(clip["frames"][:GOP])
    print("denoise log:", log["denoise"])
    assert len(handed) == 1 and np.array_equal(handed[0], want)          # the cube of the fit was given the filtered frames of the range
    assert log["denoise"] == want_log and log["denoise"]["source"] == "auto" and set(log["denoise"]) == {"sigma", "q", "source", "gain", "psnr_y"}
    assert 20.0 < log["denoise"]["psnr_y"] < 80.0 and not np.array_equal(want, clip["frames"][:GOP])          # (the filter did something)
    bs = B.parse_bitstream(blob)
    res = B.decode_video(bs, B.NullSink(), fmt=FMT, strict=True)
    assert res["verified"] and res["frames_verified"] == GOP and res["frames_mismatched"] == 0
    # GRAN: the statistics of the ORIGINAL source against the decoder's frames, not those of the filtered one
    assert bs.grain is not None and log["sections"]["GRAN"] == 122
    plain = B.parse_bitstream(B.with_grain(blob, None))
    original = grain_statistics(plain, clip["frames"][:GOP], H, W, FMT, dev, flat_threshold=65535, max_residual=255)
    filtered = grain_statistics(B.parse_bitstream(B.with_grain(blob, None)), want, H, W, FMT, dev, flat_threshold=65535, max_residual=255)
    assert original != filtered
    assert fit_grain(original, 5, source=bs.grain.source) == bs.grain and fit_grain(filtered, 5, source=bs.grain.source) != bs.grain
    assert log["grain"]["scale"] == [list(r) for r in bs.grain.scale]
    # the cube the fit was given holds the filtered frames; without the keyword it holds the file's
    cube = VideoFileCube(clip["path"], device=dev, resident="u8", frame_range=(0, GOP), frames=want)
    assert np.array_equal(cube._u8.cpu().numpy(), want) and cube.len_z_frames == GOP
    assert np.array_equal(VideoFileCube(clip["path"], device=dev, resident="u8", frame_range=(0, GOP))._u8.cpu().numpy(), clip["frames"][:GOP])
    with pytest.raises(ValueError, match="frames must be"):
        VideoFileCube(clip["path"], device=dev, frame_range=(0, GOP), frames=want[:3])


def test_without_denoise_the_log_and_the_sections_are_what_they_were(clip, handed):
    from gsvc_amd.fit_setup import encode_gop
    dev = torch.device("cuda", 0)
    blob, log = encode_gop(clip["path"], dev, frame_range=(0, GOP), **FIT)
    assert handed == [None]                                                   # the file's own frames
    assert "denoise" not in log and "grain" not in log
    assert set(log) == {"W", "H", "frames", "steps", "init", "anchors_initial", "loss_domain", "loss_matrix", "distortion", "anchors_coded",
                        "fit_seconds", "hash_format", "verify_decode_fps", "sections"}
    assert set(log["sections"]) == {"HEAD", "MLPS", "ANCH", "MASK", "HASH", "SLAB", "PHSH"}
    assert B.decode_video(B.parse_bitstream(blob), B.NullSink(), fmt=FMT, strict=True)["frames_verified"] == GOP
    given, glog = encode_gop(clip["path"], dev, frame_range=(0, GOP), denoise=2.0, denoise_gain=1.5, **FIT)
    assert glog["denoise"]["source"] == "given" and glog["denoise"]["q"] == [48, 48, 48] and glog["denoise"]["gain"] == 1.5
    assert set(glog) == set(log) | {"denoise"} and set(glog["sections"]) == set(log["sections"])
    rgb = str(clip["tmp"] / "clip.rgb")
    with open(rgb, "wb") as f:
        f.write(bytes(3 * H * W * 2))
    with pytest.raises(ValueError, match="rgb24"):                                            # refused before the fit starts
        encode_gop(rgb, dev, video_size=(W, H), denoise="auto", **FIT)
    for bad in ((4, 4), (0, T + 1), (-1, 4), (3,)):                                           # a bad range is named as one, before anything is filtered
        with pytest.raises(ValueError, match="frame_range"):
            encode_gop(clip["path"], dev, frame_range=bad, denoise="auto", **FIT)


def test_the_encode_tool_filters_every_gop_on_its_own(clip, capsys, handed):
    import gsvc_encode
    coded = str(clip["tmp"] / "clip.gsvs")
    log = gsvc_encode.main([clip["path"], "-o", coded, "--gop-frames", "8", "--denoise", "2.0"] + FIT_ARGS)
    assert [(g["first"], g["frames"]) for g in log["gops"]] == [(0, GOP), (GOP, GOP)]
    first, log_a = _filtered(clip["frames"][:GOP], sigma=2.0)
    second, log_b = _filtered(clip["frames"][GOP:], sigma=2.0)
    whole, _ = _filtered(clip["frames"], sigma=2.0)
    assert len(handed) == 2 and np.array_equal(handed[0], first) and np.array_equal(handed[1], second)          # what the two fits were given
    assert [g["denoise"] for g in log["gops"]] == [log_a, log_b] and log_a["psnr_y"] != log_b["psnr_y"]
    # a filter that saw the other side of the cut would have given other frames next to it, and another PSNR
    assert not np.array_equal(whole[GOP], second[0]) and not np.array_equal(whole[GOP - 1], first[GOP - 1])
    assert np.array_equal(whole[:GOP - 2], first[:GOP - 2]) and np.array_equal(whole[GOP + 2:], second[2:])          # radius 2: further away nothing differs
    res = S.decode_sequence(coded, B.NullSink(), strict=True)
    assert res["frames_verified"] == T


def test_the_denoise_tool_writes_what_denoise_frames_returns(clip, capsys):
    import json

    import denoise_video
    out = str(clip["tmp"] / "filtered.y4m")
    capsys.readouterr()
    log = denoise_video.main([clip["path"], out, "--gop-frames", "8", "--chunk", "3"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["frames"] == T
    hdr, got = read_y4m(out)
    assert (hdr["W"], hdr["H"], hdr["fps"], hdr["layout"], hdr["depth"]) == (W, H, (25, 1), "yuv420p", 8) and got.shape == (T, NB)
    first, log_a = _filtered(clip["frames"][:GOP])
    second, log_b = _filtered(clip["frames"][GOP:])
    assert np.array_equal(got, np.concatenate([first, second]))                                # (whatever the chunk)
    assert log["ranges"] == [dict(first=0, stop=GOP, **log_a), dict(first=GOP, stop=T, **log_b)] and log["format"] == "yuv420p"
    # one range, a given sigma
    one = str(clip["tmp"] / "one.yuv")
    log = denoise_video.main([clip["path"], one, "--sigma", "2", "--gain", "1.5"])
    whole, log_w = _filtered(clip["frames"], sigma=2.0, gain=1.5)
    assert np.array_equal(np.fromfile(one, np.uint8).reshape(T, NB), whole) and log["ranges"] == [dict(first=0, stop=T, **log_w)]
    with pytest.raises(ValueError, match="tile"):
        TF.denoise_video(clip["path"], one, frame_ranges=[(0, 8), (9, 16)])
