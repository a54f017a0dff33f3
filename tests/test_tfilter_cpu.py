"""CPU tests of the temporal prefilter (gsvc_amd/tfilter.py): properties of the numpy restatement of its docstring
(tests/_tfilter_ref.py) — it removes noise where the prediction fits, rejects a neighbour where it does not, and returns its input where
nothing is to be done —, the pinned default tables, the rounding of the vectors, the host side of the noise estimate, the options of
the three tools and the refusals that need no device.  The GPU tests hold the kernel to this reference bit for bit.

The clip of the properties is 70 x 100, 8-bit: a smooth pattern with one bright rectangle, five frames, the middle one the target."""
import math
import os
import sys

import numpy as np
import pytest

from gsvc_amd import tfilter as TF
from gsvc_amd.frames_out import FrameFormat
from tests import _tfilter_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, T = 70, 100, 5
LUT_B, LUT_P = TF.default_luts()


def _clip(sigma: float, speed: float, seed: int):
    """(clean [T, H, W] int64, noisy [T, H, W] int64): the pattern moving ``speed`` pixels per frame to the right, Gaussian noise added."""
    rng = np.random.default_rng(seed)
    clean = np.stack([np.rint(ref.pattern(H, W, speed * t)) for t in range(T)]).astype(np.int64)
    noisy = np.clip(np.rint(clean + rng.normal(0.0, sigma, clean.shape)), 0, 255).astype(np.int64)
    return clean, noisy


def _filter_middle(noisy, flow_x: float, q: int, wt=TF.DEFAULT_WT):
    """The filtered luma of frame 2 of a yuv444p clip whose chroma planes repeat the luma; the flow to frame 2 + d is (d flow_x, 0)."""
    clip = [(p, p, p) for p in noisy]
    flows = {d: np.stack([np.full((H, W), d * flow_x, np.float32), np.zeros((H, W), np.float32)]) for d in ref.OFFSETS}
    return ref.filter_planes(clip, 2, flows, (q, q, q), wt, LUT_B, LUT_P, "yuv444p")


def _mse(a, b, margin: int = 0):
    d = (np.asarray(a, np.float64) - np.asarray(b, np.float64))[margin:H - margin, margin:W - margin]
    return float((d * d).mean())


@pytest.mark.parametrize("sigma", [1.5, 3.0, 6.0])
def test_static_clip_with_zero_flow_loses_at_least_half_its_noise(sigma):
    clean, noisy = _clip(sigma, 0.0, seed=int(10 * sigma))
    out = _filter_middle(noisy, 0.0, int(round(16 * sigma)))
    ratio = _mse(out[0], clean[2]) / _mse(noisy[2], clean[2])
    print(f"static, sigma {sigma}: output MSE / input MSE = {ratio:.3f}")
    assert ratio <= 0.5
    assert np.array_equal(out[1], out[0]) and np.array_equal(out[2], out[0])          # (4:4:4 chroma that repeats the luma is filtered alike)


def test_moving_content_with_a_wrong_flow_is_rejected():
    clean, noisy = _clip(3.0, 3.0, seed=5)
    out = _filter_middle(noisy, 0.0, 48)
    ratio = _mse(out[0], clean[2]) / _mse(noisy[2], clean[2])
    print(f"moving 3 px per frame, zero flow: output MSE / input MSE = {ratio:.3f}")
    assert ratio <= 1.05


def test_moving_content_with_the_true_flow_loses_at_least_half_its_noise():
    clean, noisy = _clip(3.0, 3.0, seed=6)
    out = _filter_middle(noisy, 3.0, 48)
    ratio = _mse(out[0], clean[2], margin=8) / _mse(noisy[2], clean[2], margin=8)
    print(f"moving 3 px per frame, true flow: output MSE / input MSE in the interior = {ratio:.3f}")
    assert ratio <= 0.5


@pytest.mark.parametrize("layout", ["yuv420p", "yuv444p"])
def test_identical_frames_and_zero_weights_return_the_input(layout):
    rng = np.random.default_rng(3)
    ch, cw = (H // 2, W // 2) if layout == "yuv420p" else (H, W)
    frame = (rng.integers(0, 256, (H, W)), rng.integers(0, 256, (ch, cw)), rng.integers(0, 256, (ch, cw)))
    flows = {d: np.zeros((2, H, W), np.float32) for d in ref.OFFSETS}
    same = ref.filter_planes([frame] * T, 2, flows, (16, 16, 16), TF.DEFAULT_WT, LUT_B, LUT_P, layout)
    assert all(np.array_equal(a, b) for a, b in zip(same, frame))
    other = [tuple(rng.integers(0, 256, p.shape) for p in frame) for _ in range(T)]
    wild = {d: rng.uniform(-9, 9, (2, H, W)).astype(np.float32) for d in ref.OFFSETS}
    off = ref.filter_planes(other, 2, wild, (65535, 65535, 65535), (0, 0), LUT_B, LUT_P, layout)
    assert all(np.array_equal(a, b) for a, b in zip(off, other[2]))
    on = ref.filter_planes(other, 2, wild, (65535, 65535, 65535), TF.DEFAULT_WT, LUT_B, LUT_P, layout)
    assert not np.array_equal(on[0], other[2][0])                                      # (and with weights it does something)
    # a clip of one frame has no neighbour
    alone = ref.filter_planes([frame], 0, {}, (16, 16, 16), TF.DEFAULT_WT, LUT_B, LUT_P, layout)
    assert all(np.array_equal(a, b) for a, b in zip(alone, frame))


def test_default_tables_are_pinned():
    assert len(LUT_B) == len(LUT_P) == 64
    assert [LUT_B[i] for i in (0, 16, 17, 24, 63)] == [256, 256, 226, 94, 1]
    assert [LUT_P[i] for i in (0, 16, 17, 24, 63)] == [256, 205, 199, 155, 8]
    assert (list(LUT_B), list(LUT_P)) == tuple(ref.luts())
    assert all(a >= b for a, b in zip(LUT_B, LUT_B[1:])) and all(a >= b for a, b in zip(LUT_P, LUT_P[1:]))
    p = TF.TemporalFilterParams()
    assert p.wt == (128, 64) and p.lut_b == LUT_B and p.lut_p == LUT_P and p.radius == 2
    for bad in (dict(radius=3), dict(wt=(128,)), dict(wt=(257, 0)), dict(lut_b=(1,) * 63), dict(lut_p=(300,) * 64), dict(wt=(-1, 0))):
        with pytest.raises(ValueError):
            TF.TemporalFilterParams(**bad)


def test_vectors_round_half_to_even_and_clamp():
    f = np.array([0.125, -0.125, 0.375, -0.375, 0.625, 0.1249, 1e9, -1e9, 8191.75, 8192.0, -8192.0, -8192.25], np.float32).reshape(1, 1, -1)
    assert ref.vectors(np.concatenate([f, f]))[0, 0].tolist() == [0, 0, 2, -2, 2, 0, 32767, -32768, 32767, 32767, -32768, -32768]
    # through the filter: a flow of 0.125 samples where a flow of 0 does, one of 0.375 where 0.5 does
    rng = np.random.default_rng(8)
    clip = [tuple(rng.integers(0, 256, (16, 24)) for _ in range(3)) for _ in range(3)]

    def run(fx):
        flows = {d: np.stack([np.full((16, 24), fx, np.float32), np.full((16, 24), -fx, np.float32)]) for d in ref.OFFSETS}
        return ref.filter_planes(clip, 1, flows, (4000, 4000, 4000), TF.DEFAULT_WT, LUT_B, LUT_P, "yuv444p")

    zero, half = run(0.0), run(0.5)
    assert all(np.array_equal(a, b) for a, b in zip(run(0.125), zero)) and all(np.array_equal(a, b) for a, b in zip(run(-0.125), zero))
    assert all(np.array_equal(a, b) for a, b in zip(run(0.375), half)) and not np.array_equal(half[0], zero[0])


def test_noise_strength_on_given_sums():
    fmt = FrameFormat("yuv444p")
    # 10 x 10: 64 interior samples; S = 384 = 6 x 64 makes sigma sqrt(pi / 2) exactly
    sigma, q = TF.noise_strength([[384, 384, 768]], 10, 10, fmt)
    assert sigma == pytest.approx((math.sqrt(math.pi / 2),) * 2 + (2 * math.sqrt(math.pi / 2),), rel=1e-12) and q == (20, 20, 40)
    assert TF.noise_strength([[384, 384, 768], [0, 0, 0]], 10, 10, fmt, gain=2.0)[1] == (20, 20, 40)          # two frames: the mean; gain 2
    assert TF.noise_strength([[0, 0, 0]], 10, 10, fmt)[1] == (1, 1, 1) and TF.noise_strength([[1 << 50] * 3], 10, 10, fmt)[1] == (65535,) * 3
    # 4:2:0: the chroma planes have their own interior
    assert TF.interior_samples(16, 24, FrameFormat("yuv420p")) == (14 * 22, 6 * 10, 6 * 10)
    s420, _ = TF.noise_strength([[6 * 14 * 22, 6 * 60, 12 * 60]], 16, 24, FrameFormat("yuv420p"))
    assert s420 == pytest.approx((math.sqrt(math.pi / 2),) * 2 + (2 * math.sqrt(math.pi / 2),), rel=1e-12)


@pytest.mark.parametrize("sigma", [1.5, 3.0, 6.0])
def test_noise_estimate_of_the_test_picture_is_within_15_percent(sigma):
    _, noisy = _clip(sigma, 0.0, seed=int(100 * sigma))
    frames = ref.clip_444(noisy)
    sums = ref.noise_sums_ref(frames, H, W, "yuv444p", 8)
    assert sums.shape == (T, 3) and np.array_equal(sums[:, 0], sums[:, 1])
    got, q = TF.noise_strength(sums, H, W, FrameFormat("yuv444p"))
    print(f"noise estimate for sigma {sigma}: {got[0]:.3f}, q {q[0]}")
    assert abs(got[0] - sigma) <= 0.15 * sigma and q[0] == int(round(16 * got[0]))
    assert ref.noise_sums_ref(np.full((1, 3 * H * W), 77, np.uint8), H, W, "yuv444p", 8).tolist() == [[0, 0, 0]]


def test_the_tools_take_the_denoise_options(capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import denoise_video
    import fit_synthetic
    import gsvc_encode
    a = gsvc_encode.parse_args(["clip.y4m", "-o", "clip.gsvc", "--denoise", "auto", "--gop-frames", "8"])
    assert a.denoise == "auto" and a.denoise_gain is None and a.gop_frames == 8
    a = gsvc_encode.parse_args(["clip.y4m", "-o", "clip.gsvc", "--denoise", "2.5", "--denoise-gain", "1.5", "--film-grain"])
    assert a.denoise == 2.5 and a.denoise_gain == 1.5 and a.film_grain
    assert gsvc_encode.parse_args(["clip.y4m", "-o", "clip.gsvc"]).denoise is None
    a = fit_synthetic.parse_args(["--video", "clip.y4m", "--denoise", "auto"])
    assert a.denoise == "auto" and fit_synthetic.parse_args([]).denoise is None
    a = denoise_video.parse_args(["in.y4m", "out.y4m"])
    assert a.sigma == "auto" and a.gain == 1.0 and a.gop_frames is None and a.chunk == 8
    a = denoise_video.parse_args(["in.yuv", "out.yuv", "--sigma", "3", "--gain", "0.5", "--video-size", "64x48", "--gop-frames", "8", "--scene-cuts"])
    assert a.sigma == 3.0 and a.gain == 0.5 and a.video_size == "64x48" and a.gop_frames == 8 and a.scene_cuts
    for tool, argv in ((gsvc_encode, ["clip.y4m", "-o", "clip.gsvc", "--denoise-gain", "2"]), (gsvc_encode, ["clip.y4m", "-o", "clip.gsvc", "--denoise", "soft"]),
                       (gsvc_encode, ["clip.y4m", "-o", "clip.gsvc", "--denoise", "-1"]), (gsvc_encode, ["clip.y4m", "-o", "clip.gsvc", "--denoise", "0"]),
                       (fit_synthetic, ["--denoise", "auto"]), (fit_synthetic, ["--video", "clip.y4m", "--denoise-gain", "2"]),
                       (denoise_video, ["in.y4m", "out.y4m", "--sigma", "nan"]), (denoise_video, ["in.y4m", "out.y4m", "--scene-cuts"]),
                       (denoise_video, ["in.y4m", "out.png"]), (denoise_video, ["in.y4m", "out.y4m", "--gain", "0"]), (denoise_video, ["in.y4m"])):
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        assert e.value.code == 2, argv
    assert "--denoise" in capsys.readouterr().err
    assert TF.parse_sigma("auto") == "auto" and TF.parse_sigma(None) is None and TF.parse_sigma("0.75") == 0.75


def test_rgb24_and_a_zero_strength_are_refused_before_anything_runs():
    zero_flows = None          # (never looked at: the refusals come first)
    with pytest.raises(ValueError, match="rgb24"):
        TF.temporal_filter(None, 16, 24, FrameFormat("rgb24"), zero_flows, (16, 16, 16))
    with pytest.raises(ValueError, match="rgb24"):
        TF.noise_sums(None, 16, 24, FrameFormat("rgb24"))
    with pytest.raises(ValueError, match="rgb24"):
        TF.denoise_frames(None, 16, 24, FrameFormat("rgb24"))
    with pytest.raises(ValueError, match="rgb24"):
        TF.noise_strength([[0, 0, 0]], 16, 24, FrameFormat("rgb24"))
    for q in ((0, 16, 16), (16, 16, 0), 0, (16, 16), (16, 16, 65536), -3):
        with pytest.raises(ValueError, match="q is"):
            TF.temporal_filter(None, 16, 24, FrameFormat("yuv420p"), zero_flows, q)
    with pytest.raises(ValueError, match="8 x 8"):
        TF.temporal_filter(None, 6, 24, FrameFormat("yuv420p"), zero_flows, 16)
    with pytest.raises(ValueError, match="sigma"):
        TF.denoise_frames(None, 16, 24, FrameFormat("yuv420p"), sigma="strong")
    assert TF.check_q(16) == (16, 16, 16) and TF.q_of_sigma((1.5, 0.0, 1e9)) == (24, 1, 65535)
