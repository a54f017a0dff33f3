"""GPU tests of the metric kernels (csrc/metrics.hip) and what is built on them (gsvc_amd/metrics.py, report.evaluate(code_metrics=True)).

  * gsvc_frames_sse: bit-equal to the int64 NumPy sum of tests/_metrics_ref.py — every layout and depth, frames smaller than a vector, a
    plane boundary inside a vector, strides with guard bytes, the edge path against the wide path, the largest possible squares.
  * gsvc_msssim: every one of the 5 P per-scale means and the final value against the float64 statement on all 36 seeded pictures of
    tests/_metrics_ref.py, held to TWICE the error the float32 tensor expressions (``metrics.ms_ssim``'s arithmetic on the CPU) make on
    exactly these pictures: TERM_BOUND = 1.74e-4, VALUE_BOUND = 7.4e-5 (derivation there).  Codes read in place give the bits of the
    float path; two runs give the same bits.
GSVC_PRINT_ERRORS=1 prints each measured figure before it is asserted."""
import os

import numpy as np
import pytest
import torch

from gsvc_amd import frames_out as fo
from gsvc_amd import metrics
from gsvc_amd.frames_in import open_video
from gsvc_amd.frames_out import FrameFormat
from tests import _metrics_ref as ref

pytestmark = pytest.mark.gpu
FORMATS = [("rgb24", 8), ("yuv444p", 8), ("yuv420p", 8), ("yuv444p", 10), ("yuv420p", 10), ("yuv444p", 16), ("yuv420p", 16)]
SIZES = ((2, 2), (6, 10), (18, 34), (64, 64))          # H x W: the smallest 4:2:0 frame; H W = 60: U starts inside a vector; ...


def _say(what, value):
    if os.environ.get("GSVC_PRINT_ERRORS"):
        print(f"{what}: {value}")


def _random_frames(rng, n, H, W, fmt):
    """uint8 [n, frame_bytes] of random codes below 2^depth (deep: little-endian words)."""
    nb = fo.frame_bytes(H, W, fmt)
    if fmt.depth == 8:
        return rng.integers(0, 256, (n, nb), dtype=np.uint8)
    return rng.integers(0, 1 << fmt.depth, (n, nb // 2), dtype=np.uint16).astype("<u2").view(np.uint8).reshape(n, nb)


def _placed(frames, stride, offset, guard):
    """The frames on the device in a buffer of ``guard`` bytes: frame k at offset + k * stride.  -> the [n, stride] view."""
    n, nb = frames.shape
    buf = torch.full((offset + n * stride + 32,), guard, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + n * stride].view(n, stride)
    view[:, :nb] = torch.from_numpy(frames).cuda()
    return view


# ---- plane SSE ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,depth", FORMATS, ids=[f"{l}-{d}" for l, d in FORMATS])
def test_plane_sse_is_exact(layout, depth):
    fmt = FrameFormat(layout, depth=depth)
    rng = np.random.default_rng(depth + len(layout))
    off = 2 if depth > 8 else 1
    for H, W in SIZES:
        nb = fo.frame_bytes(H, W, fmt)
        for n in (1, 3, 17):
            a, b = _random_frames(rng, n, H, W, fmt), _random_frames(rng, n, H, W, fmt)
            want = ref.sse_ref(a, b, H, W, layout, depth)
            plain = metrics.plane_sse(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), H, W, fmt)
            assert plain.dtype == torch.int64 and tuple(plain.shape) == (n, 3)
            assert np.array_equal(plain.cpu().numpy(), want), (H, W, n, "tight")
            # a stride above the frame (a multiple of 16: the wide path for n > 1 too); the guard bytes differ between a and b
            stride = -(-nb // 16) * 16 + 16
            wide = metrics.plane_sse(_placed(a, stride, 0, 0x5A), _placed(b, stride, 0, 0xA5), H, W, fmt)
            assert np.array_equal(wide.cpu().numpy(), want), (H, W, n, "stride")
            # the base moved by one sample: the edge path, the same bits
            edge = metrics.plane_sse(_placed(a, stride, off, 0x5A), _placed(b, stride, off, 0xA5), H, W, fmt)
            assert torch.equal(edge, wide), (H, W, n, "edge")
            # one side only moved: still the edge path
            mixed = metrics.plane_sse(_placed(a, stride, 0, 0x11), _placed(b, stride + 2, off, 0x22), H, W, fmt)
            assert torch.equal(mixed, wide), (H, W, n, "mixed")


@pytest.mark.parametrize("layout", ["yuv444p", "yuv420p"])
def test_plane_sse_of_the_largest_squares(layout):
    """All-zero against all-65535 at 16 bits on 64 x 64: every squared difference is 4 294 836 225, just under 2^32."""
    fmt = FrameFormat(layout, depth=16)
    nb = fo.frame_bytes(64, 64, fmt)
    a = torch.zeros((2, nb), dtype=torch.uint8, device="cuda")
    b = torch.full((2, nb), 255, dtype=torch.uint8, device="cuda")
    chroma = 4096 // 4 if layout == "yuv420p" else 4096
    got = metrics.plane_sse(a, b, 64, 64, fmt).cpu().tolist()
    assert got == [[4096 * 65535 ** 2, chroma * 65535 ** 2, chroma * 65535 ** 2]] * 2
    assert got[0][0] > 2 ** 43          # far beyond what a 32-bit sum holds


@pytest.mark.parametrize("layout,depth", [("rgb24", 8), ("yuv420p", 8), ("yuv420p", 10)])
def test_equal_frames_give_zero_and_infinite_psnr(layout, depth):
    fmt = FrameFormat(layout, depth=depth)
    a = torch.from_numpy(_random_frames(np.random.default_rng(3), 3, 18, 34, fmt)).cuda()
    r = metrics.code_metrics(a, a.clone(), 18, 34, fmt)
    assert int(r["sse"].abs().sum()) == 0 and r["peak"] == float(2 ** depth - 1)
    names = ("r", "g", "b") if layout == "rgb24" else ("y", "u", "v")
    for key in [f"psnr_{c}" for c in names] + ["psnr_avg"] + (["psnr_611"] if layout == "yuv420p" else []):
        assert r[key].dtype == torch.float64 and torch.isinf(r[key]).all() and (r[key] > 0).all(), key
    assert "msssim_y" not in r          # 18 x 34: too small for five scales
    assert ("psnr_611" in r) == (layout == "yuv420p")


def test_code_metrics_follow_the_conventions():
    fmt = FrameFormat("yuv420p", depth=10)
    H, W, n = 18, 34, 3
    rng = np.random.default_rng(11)
    a, b = _random_frames(rng, n, H, W, fmt), _random_frames(rng, n, H, W, fmt)
    r = metrics.code_metrics(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), H, W, fmt)
    sse = ref.sse_ref(a, b, H, W, "yuv420p", 10)
    assert np.array_equal(r["sse"].cpu().numpy(), sse)
    counts = (H * W, H * W // 4, H * W // 4)
    planes = [ref.psnr_ref(sse[:, k], counts[k], 1023.0) for k in range(3)]
    for k, c in enumerate("yuv"):
        assert np.allclose(r[f"psnr_{c}"].cpu().numpy(), planes[k], rtol=0, atol=1e-12)
    assert np.allclose(r["psnr_avg"].cpu().numpy(), ref.psnr_ref(sse.sum(1), sum(counts), 1023.0), rtol=0, atol=1e-12)
    assert np.allclose(r["psnr_611"].cpu().numpy(), (6 * planes[0] + planes[1] + planes[2]) / 8, rtol=0, atol=1e-12)


# ---- fused MS-SSIM -----------------------------------------------------------------------------------------------------------
def _floats(codes):
    """uint8 codes -> float32 CUDA code / 255 (the division on the host: an IEEE division)."""
    return torch.from_numpy(codes.astype(np.float32) / np.float32(255.0)).cuda()


@pytest.mark.parametrize("case", ref.CASES, ids=[f"{'x'.join(str(v) for v in ref.SHAPES[s])}-{f}-{g}" for s, f, g in ref.CASES])
def test_msssim_fused_against_float64(case):
    x, y = ref.picture_codes(*case)
    want_t, want_v = ref.reference(*case)
    value, terms = metrics.ms_ssim_fused(_floats(x), _floats(y), size_average=False, terms=True)
    assert terms.dtype == torch.float64 and tuple(terms.shape) == (5,) + x.shape[:2] and value.dtype == torch.float64
    err_t = np.abs(terms.cpu().numpy() - want_t).max(axis=(1, 2))
    err_v = float(np.abs(value.cpu().numpy() - want_v.mean(1)).max())
    _say(f"msssim {case} term errors per scale", err_t.tolist())
    _say(f"msssim {case} value error", err_v)
    assert err_t.max() <= ref.TERM_BOUND
    per_plane = np.abs(metrics._msssim_value(terms).cpu().numpy() - want_v).max()
    assert per_plane <= ref.VALUE_BOUND and err_v <= ref.VALUE_BOUND
    mean = float(metrics.ms_ssim_fused(_floats(x), _floats(y)))
    assert abs(mean - float(want_v.mean())) <= ref.VALUE_BOUND


@pytest.mark.parametrize("shape_id", range(len(ref.SHAPES)))
def test_msssim_fused_identity_repeat_and_agreement_with_the_tensor_expressions(shape_id):
    for family, sigma in (("smooth", 0.02), ("uniform", 0.1), ("flat", 0.002)):
        x, y = ref.picture_codes(shape_id, family, sigma)
        fx, fy = _floats(x), _floats(y)
        one, t_one = metrics.ms_ssim_fused(fx, fx, terms=True)
        _say(f"msssim identity {shape_id} {family}", abs(float(one) - 1.0))
        assert abs(float(one) - 1.0) <= 1e-6 and float((t_one - 1.0).abs().max()) <= 1e-6
        v1, t1 = metrics.ms_ssim_fused(fx, fy, size_average=False, terms=True)
        v2, t2 = metrics.ms_ssim_fused(fx, fy, size_average=False, terms=True)
        assert torch.equal(t1, t2) and torch.equal(v1, v2)          # the same bits
        plain = float(metrics.ms_ssim(fx, fy))
        fused = float(metrics.ms_ssim_fused(fx, fy))
        _say(f"msssim fused - tensor expressions {shape_id} {family} {sigma}", abs(plain - fused))
        assert abs(plain - fused) <= ref.VALUE_BOUND + ref.VALUE_BOUND          # each within its bound of the float64 value
    if ref.SHAPES[shape_id][1] == 1:          # a [C, H, W] picture is a batch of one
        assert float(metrics.ms_ssim_fused(fx[0], fy[0])) == fused


def test_msssim_refuses_small_pictures_on_the_device():
    z = torch.zeros((1, 1, 160, 200), device="cuda")
    with pytest.raises(ValueError, match="exceed 160"):
        metrics.ms_ssim_fused(z, z)
    with pytest.raises(ValueError):
        metrics.ms_ssim_fused(torch.zeros((1, 1, 200, 200), device="cuda"), torch.zeros((1, 2, 200, 200), device="cuda"))


@pytest.mark.parametrize("depth", [8, 10])
def test_msssim_on_codes_in_place_equals_the_float_path(depth):
    """The Y planes of a yuv420p / yuv420p10le buffer (row pitch W, plane pitch = the frame stride, with guard bytes behind every frame)
    against the float path on code / peak planes: the same bits."""
    fmt = FrameFormat("yuv420p", depth=depth)
    H, W = ref.SHAPES[2][2:]          # 162 x 330: even sides
    peak = float(2 ** depth - 1)
    rng = np.random.default_rng(depth)
    ya, yb = [], []
    for sigma in (0.02, 0.1):
        x, y = ref.picture_codes(2, "smooth", sigma)
        up = 1 << (depth - 8)
        ya.append(x[0, 0].astype(np.int64) * up + rng.integers(0, up, (H, W)))
        yb.append(y[0, 0].astype(np.int64) * up + rng.integers(0, up, (H, W)))
    ya, yb = np.stack(ya), np.stack(yb)          # [2, H, W] codes below 2^depth
    frames = []
    for codes in (ya, yb):
        fr = _random_frames(rng, 2, H, W, fmt)
        if depth == 8:
            fr[:, :H * W] = codes.reshape(2, -1).astype(np.uint8)
        else:
            fr[:, :2 * H * W] = codes.reshape(2, -1).astype("<u2").view(np.uint8).reshape(2, -1)
        frames.append(fr)
    nb = fo.frame_bytes(H, W, fmt)
    a, b = _placed(frames[0], nb + 48, 0, 0x5A), _placed(frames[1], nb + 80, 0, 0xA5)          # two strides, guards that differ
    r = metrics.code_metrics(a, b, H, W, fmt)
    fx = torch.from_numpy(ya.astype(np.float32) / np.float32(peak)).cuda().unsqueeze(1)
    fy = torch.from_numpy(yb.astype(np.float32) / np.float32(peak)).cuda().unsqueeze(1)
    want = metrics.ms_ssim_fused(fx, fy, size_average=False)
    assert r["msssim_y"].dtype == torch.float64 and tuple(r["msssim_y"].shape) == (2,)
    assert torch.equal(r["msssim_y"], want)
    assert 0.5 < float(want.min()) < 1.0
    tight = metrics.code_metrics(torch.from_numpy(frames[0]).cuda(), torch.from_numpy(frames[1]).cuda(), H, W, fmt, msssim=False)
    assert "msssim_y" not in tight and torch.equal(tight["sse"], r["sse"])


def test_msssim_of_rgb24_frames_is_the_mean_over_the_channels():
    H, W = 162, 176
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (2, H, W, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    r = metrics.code_metrics(torch.from_numpy(a.reshape(2, -1)).cuda(), torch.from_numpy(b.reshape(2, -1)).cuda(), H, W, FrameFormat("rgb24"))
    want = metrics.ms_ssim_fused(_floats(a.transpose(0, 3, 1, 2)), _floats(b.transpose(0, 3, 1, 2)), size_average=False)
    assert torch.equal(r["msssim_y"], want)


# ---- on top: evaluate and compare_videos ------------------------------------------------------------------------------------------
H2, W2 = 162, 176


def test_evaluate_with_code_metrics(tmp_path):
    from gsvc_amd.report import evaluate
    from tests.test_train_gpu import _setup
    pc, cube, opt, pipe, mp, Trainer = _setup(anchors=3000, H=H2, W=W2)
    opt.full_precision_training_total = 1000
    pc.training_setup(opt)
    tr = Trainer(pc, cube, opt, pipe, mp)
    for it in range(1, 5):          # a few fitting steps, so that the frames are not flat
        tr.step(it)
    bg, ids, fmt = torch.zeros(3), [3, 4], FrameFormat("yuv420p")
    plain = evaluate(pc, cube, pipe, bg, frame_ids=ids, delivered=fmt)
    ev = evaluate(pc, cube, pipe, bg, frame_ids=ids, delivered=fmt, code_metrics=True)
    new = ["msssim_y", "psnr_611", "psnr_avg", "psnr_u", "psnr_v", "psnr_y"]
    assert sorted(set(ev) - set(plain)) == new
    for k in plain:
        if k != "fps":
            assert ev[k] == plain[k], k
    assert 5.0 < ev["psnr_y"] < 100.0 and 0.0 < ev["msssim_y"] <= 1.0
    # the numbers are code_metrics of the two frame buffers
    from gsvc_amd.ortho_gaussian_renderer import render_frames
    frames = [cube[i] for i in ids]
    dec = fo.frames_to_u8([torch.clamp(img, 0.0, 1.0) for img in render_frames(frames, pc, pipe, bg, batch=8)], fmt)
    src = fo.frames_to_u8([torch.clamp(fr.image.cuda(), 0.0, 1.0).permute(0, 2, 1).contiguous() for fr in frames], fmt)
    direct = metrics.code_metrics(dec, src, H2, W2, fmt)
    for k in new:
        assert ev[k] == float(direct[k].sum()) / 2, k
    # the source's own bytes from a file: the same numbers
    path = tmp_path / "source.y4m"
    with fo.Y4MWriter(path, W2, H2, (30, 1), fmt) as sink:
        for fr in src.cpu():
            sink.write(fr)
    hdr, from_file = open_video(path)
    again = evaluate(pc, cube, pipe, bg, frame_ids=ids, delivered=fmt, code_metrics=True, source_u8=from_file)
    for k in new:
        assert again[k] == ev[k], k
    fused = evaluate(pc, cube, pipe, bg, frame_ids=ids, delivered=fmt, msssim="fused")
    assert sorted(fused) == sorted(plain) and abs(fused["msssim"] - plain["msssim"]) <= 2 * ref.VALUE_BOUND


@pytest.mark.parametrize("depth,frames,chunk", [(8, 3, 16), (10, 5, 2)])
def test_compare_videos_equals_code_metrics_on_the_same_bytes(tmp_path, depth, frames, chunk):
    fmt = FrameFormat("yuv420p", depth=depth)
    rng = np.random.default_rng(depth)
    g = torch.Generator().manual_seed(depth)
    pics = torch.rand((frames, 3, H2 // 6, W2 // 8), generator=g)
    pics = torch.nn.functional.interpolate(pics, size=(H2, W2), mode="bilinear", align_corners=False).cuda()
    noisy = (pics + 0.03 * torch.randn(pics.shape, generator=g).cuda()).clamp(0, 1)
    a, b = fo.frames_to_u8(pics, fmt).cpu().numpy(), fo.frames_to_u8(noisy, fmt).cpu().numpy()
    del rng
    paths = []
    for name, data in (("ref.y4m", a), ("dec.y4m", b)):
        with fo.Y4MWriter(tmp_path / name, W2, H2, (30, 1), fmt) as sink:
            for fr in data:
                sink.write(fr)
        paths.append(str(tmp_path / name))
    got = metrics.compare_videos(paths[0], paths[1], chunk=chunk)
    want = metrics.code_metrics(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), H2, W2, fmt)
    assert (got["frames"], got["W"], got["H"], got["format"], got["peak"]) == (frames, W2, H2, fmt.name, float(2 ** depth - 1))
    keys = ["psnr_y", "psnr_u", "psnr_v", "psnr_avg", "psnr_611", "msssim_y"]
    assert sorted(got["per_frame"]) == sorted(keys)
    for k in keys:
        assert got["per_frame"][k] == want[k].tolist(), k
        assert got[k] == float(np.mean(np.asarray(want[k].tolist(), np.float64))), k
    total = ref.sse_ref(a, b, H2, W2, "yuv420p", depth).sum(0)
    counts = (H2 * W2, H2 * W2 // 4, H2 * W2 // 4)
    for k, c in enumerate("yuv"):
        assert abs(got[f"psnr_{c}_seq"] - float(ref.psnr_ref(total[k], counts[k] * frames, got["peak"]))) < 1e-12
    assert abs(got["psnr_avg_seq"] - float(ref.psnr_ref(total.sum(), sum(counts) * frames, got["peak"]))) < 1e-12
    assert 20.0 < got["psnr_y"] < 60.0 and 0.5 < got["msssim_y"] < 1.0
