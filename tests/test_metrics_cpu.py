"""CPU tests of the video metrics: the float64 / integer references of tests/_metrics_ref.py on values one can do by hand and against
``metrics.ms_ssim``'s arithmetic in float64, the PSNR conventions, and everything of csrc/metrics.hip and its Python side that runs
before a launch (argument checks, the workspace query, ``evaluate``'s and ``compare_videos``' refusals)."""
import ctypes as C

import numpy as np
import pytest
import torch

from gsvc_amd import _lib, metrics
from gsvc_amd.frames_out import FrameFormat, Y4MWriter, frame_bytes
from tests import _metrics_ref as ref


# ---- the reference on values one can do by hand --------------------------------------------------------------------------------
def test_reference_on_a_constant_pair():
    """Two constants a, b on 176 x 176 (even down to 11 x 11: every scale stays constant): variances and covariance vanish, cs = C2 / C2
    = 1 at every scale, and the last term is the luminance ratio alone."""
    a, b = 0.5, 0.25
    terms, value = ref.ms_ssim_ref(np.full((176, 176), a), np.full((176, 176), b))
    lum = (2 * a * b + ref.C1) / (a * a + b * b + ref.C1)
    assert np.abs(terms[:4] - 1.0).max() < 1e-12
    assert abs(terms[4] - lum) < 1e-12
    assert abs(value - lum ** 0.1333) < 1e-12
    same, one = ref.ms_ssim_ref(np.full((161, 163), 0.7), np.full((161, 163), 0.7))          # x = y: 1 whatever the pooled borders do
    assert np.abs(same - 1.0).max() < 1e-12 and abs(one - 1.0) < 1e-12


def test_reference_at_an_11x11_last_scale():
    """161 -> 81 -> 41 -> 21 -> 11: the last scale has ONE output, the full window's weighted moments, written out directly here."""
    rng = np.random.default_rng(5)
    x, y = rng.uniform(size=(161, 161)), rng.uniform(size=(161, 161))
    px, py = ref.pyramid(x)[4], ref.pyramid(y)[4]
    assert px.shape == (11, 11)
    w2 = np.outer(ref.window(), ref.window())
    mu1, mu2 = (w2 * px).sum(), (w2 * py).sum()
    s1, s2, s12 = (w2 * px * px).sum() - mu1 ** 2, (w2 * py * py).sum() - mu2 ** 2, (w2 * px * py).sum() - mu1 * mu2
    want = (2 * mu1 * mu2 + ref.C1) / (mu1 ** 2 + mu2 ** 2 + ref.C1) * (2 * s12 + ref.C2) / (s1 + s2 + ref.C2)
    terms, _ = ref.ms_ssim_ref(x, y)
    assert abs(terms[4] - want) < 1e-13
    assert abs(ref.window().sum() - 1.0) < 1e-15 and ref.window()[5] == ref.window().max()


def test_reference_pooling_of_a_3x3_plane():
    """Odd sides: one leading zero row and column, the padded cells count in the divisor."""
    got = ref.pool2(np.arange(1.0, 10.0).reshape(3, 3))
    assert np.array_equal(got, np.array([[1 / 4, (2 + 3) / 4], [(4 + 7) / 4, (5 + 6 + 8 + 9) / 4]]))
    assert np.array_equal(ref.pool2(np.arange(1.0, 9.0).reshape(2, 4)), np.array([[(1 + 2 + 5 + 6) / 4, (3 + 4 + 7 + 8) / 4]]))
    assert [p.shape for p in ref.pyramid(np.zeros((161, 330)))] == [(161, 330), (81, 165), (41, 83), (21, 42), (11, 21)]


@pytest.mark.parametrize("shape_id", range(len(ref.SHAPES)))
def test_reference_against_ms_ssim_in_float64(shape_id):
    """The NumPy statement and ``metrics.ms_ssim``'s tensor expressions on float64 tensors agree to rounding on the GPU tests' shapes,
    term by term; and ``ms_ssim`` itself (float32) lands within the measured float32 error of the reference."""
    for family, sigma in (("smooth", 0.02), ("uniform", 0.1), ("flat", 0.002)):
        x, y = ref.picture_codes(shape_id, family, sigma)
        rt, rv = ref.reference(shape_id, family, sigma)
        t, v = ref.torch_terms(torch.from_numpy(x.astype(np.float64) / 255.0), torch.from_numpy(y.astype(np.float64) / 255.0), torch.float64)
        assert np.abs(t.numpy() - rt).max() < 1e-11 and np.abs(v.numpy() - rv).max() < 1e-11
        got = float(metrics.ms_ssim(torch.from_numpy(x.astype(np.float32) / np.float32(255.0)),
                                    torch.from_numpy(y.astype(np.float32) / np.float32(255.0))))
        assert abs(got - rv.mean()) <= ref.VALUE_BOUND


def test_the_bounds_are_twice_the_measured_float32_error():
    assert ref.TERM_BOUND == 2 * ref.F32_TERM_ERROR and ref.VALUE_BOUND == 2 * ref.F32_VALUE_ERROR
    assert 0 < ref.F32_VALUE_ERROR < ref.F32_TERM_ERROR < 1e-4
    assert len(ref.CASES) == 36          # four shapes x three families x three sigmas: none dropped


# ---- SSE and the PSNR conventions ---------------------------------------------------------------------------------------------
def test_sse_reference_by_hand():
    a = np.array([[0, 1, 2, 3, 10, 20]], np.uint8)          # 2 x 2 4:2:0: Y = 0 1 2 3, U = 10, V = 20
    b = np.array([[1, 1, 0, 7, 13, 16]], np.uint8)
    assert ref.sse_ref(a, b, 2, 2, "yuv420p", 8).tolist() == [[1 + 0 + 4 + 16, 9, 16]]
    rgb_a, rgb_b = np.array([[1, 2, 3, 4, 5, 6]], np.uint8), np.array([[0, 0, 0, 0, 0, 0]], np.uint8)          # 1 x 2 rgb24
    assert ref.sse_ref(rgb_a, rgb_b, 1, 2, "rgb24", 8).tolist() == [[1 + 16, 4 + 25, 9 + 36]]
    deep_a = np.array([[0xFF, 0xFF] * 12], np.uint8)          # 2 x 2 4:4:4 at 16 bits, every code 65535, against zeros
    assert ref.sse_ref(deep_a, np.zeros_like(deep_a), 2, 2, "yuv444p", 16).tolist() == [[4 * 65535 ** 2] * 3]


def test_psnr_conventions():
    """peak = 2^d - 1; +inf for SSE 0; 6:1:1 on the plane PSNRs; psnr_avg from the pooled SSE — through the same helpers
    ``code_metrics`` uses (they run on CPU tensors)."""
    fmt = FrameFormat("yuv420p", depth=10)
    H, W = 4, 4
    assert metrics.plane_samples(H, W, fmt) == (16, 4, 4) and metrics.plane_names(fmt) == ("y", "u", "v")
    assert metrics.plane_names(FrameFormat("rgb24")) == ("r", "g", "b") and metrics.plane_samples(2, 3, FrameFormat("yuv444p")) == (6, 6, 6)
    sse = torch.tensor([[16, 4, 0], [0, 0, 0]], dtype=torch.int64)
    peak = 1023.0
    py = metrics.psnr_of_sse(sse[:, 0], 16, peak)
    assert py.dtype == torch.float64
    assert abs(float(py[0]) - 20 * np.log10(1023.0)) < 1e-12          # MSE 1: 20 log10(peak) = 60.1975...
    assert float(py[1]) == float("inf") and float(metrics.psnr_of_sse(sse[0, 2], 4, peak)) == float("inf")
    avg = metrics.psnr_of_sse(sse.sum(1), 24, peak)
    assert abs(float(avg[0]) - 10 * np.log10(1023.0 ** 2 * 24 / 20)) < 1e-12
    assert np.allclose(ref.psnr_ref(sse.numpy()[:, 0], 16, peak), py.numpy(), rtol=0, atol=1e-12)
    assert abs(float(metrics.psnr_of_sse(torch.tensor(255 ** 2), 1, 255.0))) < 1e-12          # 8 bits: peak 255, not 256
    y, u, v = 40.0, 44.0, 48.0
    assert (6 * y + u + v) / 8 == 41.5


# ---- what runs before a launch ---------------------------------------------------------------------------------------------------
def test_sse_entry_point_validates_on_the_host():
    L = _lib.lib()
    ok = (64, 48, 128, 48, 1, 4, 4, 0, 8, 256, None)          # a, a_stride, b, b_stride, n, H, W, layout, depth, out, stream
    cases = [((None,) + ok[1:], b"NULL"), (ok[:2] + (None,) + ok[3:], b"NULL"), (ok[:9] + (None, None), b"NULL"),
             (ok[:4] + (0,) + ok[5:], b"n must be"), (ok[:7] + (3,) + ok[8:], b"unknown layout"), (ok[:8] + (7,) + ok[9:], b"depth must be"),
             (ok[:8] + (17,) + ok[9:], b"depth must be"), (ok[:8] + (10,) + ok[9:], b"rgb24 frames are 8-bit"),
             ((64, 48, 128, 48, 1, 3, 4, 2, 8, 256, None), b"even"), ((64, 47, 128, 48, 1, 4, 4, 0, 8, 256, None), b"shorter than a frame"),
             ((64, 48, 128, 47, 1, 4, 4, 0, 8, 256, None), b"shorter than a frame"),
             ((65, 96, 128, 96, 1, 4, 4, 1, 10, 256, None), b"2-byte aligned"), ((64, 97, 128, 96, 1, 4, 4, 1, 10, 256, None), b"multiple of 2"),
             ((64, 95, 128, 96, 1, 4, 4, 1, 10, 256, None), b"shorter than a frame"), ((64, 48, 128, 48, 1, 0, 4, 0, 8, 256, None), b"image size")]
    for args, msg in cases:
        assert L.gsvc_frames_sse(*args) == -1, args
        assert msg in L.gsvc_last_error(), (args, L.gsvc_last_error())


def _workspace_bytes(P, H, W):
    """The layout the header describes: the pooled pictures of both inputs per scale 1 .. 4, then one float per tile, each 256-byte padded."""
    pad = lambda v: -(-v // 256) * 256          # noqa: E731
    total, parts, h, w = 0, 0, H, W
    for s in range(5):
        if s:
            total += pad(2 * P * h * w * 4)
        parts += P * -(-(h - 10) // 32) * -(-(w - 10) // 32)
        h, w = (h + 1) // 2, (w + 1) // 2
    return total + pad(parts * 4)


def test_msssim_entry_point_validates_on_the_host():
    L = _lib.lib()
    assert L.gsvc_msssim_workspace_bytes(1, 161, 163) == _workspace_bytes(1, 161, 163)
    assert L.gsvc_msssim_workspace_bytes(6, 200, 181) == _workspace_bytes(6, 200, 181)
    assert L.gsvc_msssim_workspace_bytes(3, 1080, 1920) == _workspace_bytes(3, 1080, 1920)
    for bad in ((0, 200, 200), (1, 160, 200), (1, 200, 160), (70000, 200, 200), (1, 40000, 200)):
        assert L.gsvc_msssim_workspace_bytes(*bad) < 0, bad
    ok = (1024, 200, 40000, 2048, 200, 40000, 2, 200, 200, 0, 1.0, 4096, 512, None)
    # x, x_row, x_plane, y, y_row, y_plane, P, H, W, type, peak, workspace, out, stream

    def but(**kw):
        names = ("x", "x_row", "x_plane", "y", "y_row", "y_plane", "P", "H", "W", "type", "peak", "ws", "out", "stream")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))
    cases = [(but(x=None), b"NULL"), (but(y=None), b"NULL"), (but(ws=None), b"NULL"), (but(out=None), b"NULL"), (but(P=0), b"P must be"),
             (but(H=160), b"exceed 160"), (but(W=160), b"exceed 160"), (but(H=11, W=11), b"exceed 160"), (but(type=3), b"unknown sample type"),
             (but(type=-1), b"unknown sample type"), (but(x_row=199), b"row pitch"), (but(y_row=199), b"row pitch"),
             (but(x_plane=39999), b"plane pitch"), (but(y_plane=199 * 200 + 199), b"plane pitch"), (but(x=1026), b"not aligned"),
             (but(type=2, y=2049), b"not aligned"), (but(type=1, peak=0.0), b"peak")]
    for args, msg in cases:
        assert L.gsvc_msssim(*args) == -1, args
        assert msg in L.gsvc_last_error(), (args, L.gsvc_last_error())


def test_python_side_refuses_cpu_tensors_and_bad_shapes():
    fmt = FrameFormat("yuv420p")
    a = torch.zeros((1, frame_bytes(4, 4, fmt)), dtype=torch.uint8)
    with pytest.raises(_lib.GsvcError):
        metrics.plane_sse(a, a, 4, 4, fmt)
    with pytest.raises(_lib.GsvcError):
        metrics.code_metrics(a, a, 4, 4, fmt)
    with pytest.raises(_lib.GsvcError):
        metrics.ms_ssim_fused(torch.zeros(1, 1, 200, 200), torch.zeros(1, 1, 200, 200))
    with pytest.raises(ValueError):
        metrics.plane_sse(np.zeros((1, 24), np.uint8), a, 4, 4, fmt)
    with pytest.raises(ValueError):
        metrics.plane_sse(a, a, 3, 4, fmt)          # (frame_bytes: 4:2:0 needs even sides)


def test_evaluate_needs_delivered_for_code_metrics():
    from gsvc_amd.report import evaluate
    with pytest.raises(ValueError, match="delivered"):
        evaluate(None, None, None, None, code_metrics=True)
    with pytest.raises(ValueError, match="source_u8"):
        evaluate(None, None, None, None, source_u8=np.zeros((1, 6), np.uint8))
    with pytest.raises(ValueError, match="msssim"):
        evaluate(None, None, None, None, msssim="kernel")


def _write(path, W, H, fmt, frames):
    with Y4MWriter(path, W, H, (30, 1), fmt) as sink:
        for k in range(frames):
            sink.write(np.full(frame_bytes(H, W, fmt), k, np.uint8))
    return str(path)


def test_compare_videos_refuses_files_that_do_not_match(tmp_path):
    """Layout, depth, size and length are compared on the headers, before anything is uploaded."""
    base = _write(tmp_path / "a.y4m", 8, 4, FrameFormat("yuv420p"), 2)
    for name, (W, H, fmt, T), what in (("layout", (8, 4, FrameFormat("yuv444p"), 2), "layout"), ("depth", (8, 4, FrameFormat("yuv420p", depth=10), 2), "depth"),
                                       ("size", (4, 8, FrameFormat("yuv420p"), 2), "W"), ("height", (8, 6, FrameFormat("yuv420p"), 2), "H"),
                                       ("length", (8, 4, FrameFormat("yuv420p"), 3), "frames")):
        other = _write(tmp_path / f"{name}.y4m", W, H, fmt, T)
        with pytest.raises(ValueError, match=f"differ in {what}"):
            metrics.compare_videos(base, other)
    with pytest.raises(ValueError):
        metrics.compare_videos(base, str(tmp_path / "a.txt"))
