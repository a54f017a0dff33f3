"""The Y'CbCr loss domain on the GPU: the three kernels of csrc/yuv_loss.hip through their C entry points, ``yuv_ssim_l1`` and a
fitting step with ``loss_domain = "yuv420"``, against tests/_yuv_loss_ref.py.

Error rule (that of tests/test_loss_kernels_gpu.py): e_kernel <= 4 * e32 + 4 * eps32, both errors against the float64 reference on the
scale the case names, e32 being the error of the same reference function run in fp32 on the GPU on the same inputs.  The planes are on
a nominal [0, 1]: their scale is 1; a gradient is a sum of at most three products of the incoming gradients with constants below 1:
its scale is the largest incoming gradient.  Exact compares wherever an output is one fp32 rounding of its inputs (the planes of sample
codes, the averaged frame) or must not depend on the launch shape.  Output buffers are allocated longer than needed and pre-filled
with a NaN pattern no finite input produces.  GSVC_PRINT_ERRORS=1 prints e_kernel and e32 of every case.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _yuv_loss_ref as yr
from tests._loss_kernel_refs import EPS32, PRINT, err, ssim_window

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x7FC0BEEF            # a quiet NaN with a payload
PAD = 8
SIZES = [(2, 2), (6, 10), (18, 34), (96, 64), (160, 300)]
CASES = [("yuv420p", H, W) for H, W in SIZES] + [("yuv444p", H, W) for H, W in SIZES + [(5, 7)]]
CASE_IDS = [f"{l}-{H}x{W}" for l, H, W in CASES]


def _sentinel(n, shift=0):
    """n floats (+ PAD) of the sentinel; shift = 1 moves the base off 16-byte alignment (the kernels then take their edge path)."""
    return torch.full((n + PAD + shift,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)[shift:]


def _written(buf, n):
    """Every element of [0, n) was written, none past n."""
    bits = buf.view(torch.int32)
    return bool((bits[:n] != SENTINEL).all()) and bool((bits[n:] == SENTINEL).all())


def _untouched(buf):
    return bool((buf.view(torch.int32) == SENTINEL).all())


def _lib():
    from gsvc_amd import _lib
    return _lib, _lib.lib(), _lib.current_stream()


def _rule(tag, e_k, e32):
    if PRINT:
        print(f"YUV_ERR {tag}: kernel {e_k:.3e} fp32 statement {e32:.3e}")
    assert e_k <= 4 * e32 + 4 * EPS32, (tag, e_k, e32)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _shifted(t):
    """A copy of a float tensor whose base is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


def _images(H, W, seed, pair):
    gen = torch.Generator().manual_seed(seed)
    f = (torch.rand(3, H, W, generator=gen) * 1.2 - 0.1).cuda()
    b = (torch.rand(3, H, W, generator=gen) * 1.2 - 0.1).cuda() if pair else None
    return f, b


# ================================================================================================================ sample codes -> planes
@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("layout,H,W", CASES, ids=CASE_IDS)
def test_frames_planes_is_bit_equal_to_numpy(layout, H, W, depth):
    lb, L, st = _lib()
    samples = yr.plane_floats(H, W, layout)
    bps = 1 if depth == 8 else 2
    nbytes = samples * bps
    for rng in ("limited", "full"):
        for n in (1, 3):
            codes = yr.make_codes(H, W, layout, depth, seed=H + W + depth + n, n=n)
            want = np.stack([yr.code_planes_ref(codes[k], H, W, rng, depth) for k in range(n)])
            # placement 0: base moved by 64 bytes, stride padded to a multiple of 16 (the vector path where the sizes allow it);
            # placement 1: base moved by 1 sample and an unaligned stride, outputs 4 bytes off (the edge path)
            for place, (off, stride, shift) in enumerate([(64, (nbytes + 15) // 16 * 16 + 48, 0), (bps, nbytes + 6, 1)]):
                buf = torch.full((off + n * stride + 32,), 0xFF, dtype=torch.uint8, device="cuda")
                keep = torch.ones(buf.numel(), dtype=torch.bool)
                raw = torch.from_numpy(codes.view(np.uint8).reshape(n, nbytes)).cuda()
                for k in range(n):
                    buf[off + k * stride:off + k * stride + nbytes] = raw[k]
                    keep[off + k * stride:off + k * stride + nbytes] = False
                before = buf.clone()
                outs = [_sentinel(samples, shift) for _ in range(n)]
                ptrs = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
                lb.check(L.gsvc_frames_planes(buf.data_ptr() + off, stride, n, H, W, yr.LAYOUT_ID[layout], yr.RANGE_ID[rng], depth, ptrs, st),
                         "gsvc_frames_planes")
                for k in range(n):
                    assert _written(outs[k], samples), (rng, n, place, k)
                    got = outs[k][:samples].cpu().numpy()
                    assert np.array_equal(got.view(np.int32), want[k].view(np.int32)), (rng, n, place, k, np.abs(got - want[k]).max())
                assert torch.equal(buf, before) and bool((buf.cpu()[keep] == 0xFF).all())


def test_frames_planes_refusals():
    lb, L, st = _lib()
    H, W = 6, 10
    buf = torch.zeros(4 * 90 + 64, dtype=torch.uint8, device="cuda")
    out = _sentinel(180)
    ptrs = (C.c_void_p * 1)(out.data_ptr())
    L420, L444 = yr.LAYOUT_ID["yuv420p"], yr.LAYOUT_ID["yuv444p"]

    def refused(text, *args):
        assert L.gsvc_frames_planes(*args, ptrs, st) != 0
        msg = L.gsvc_last_error().decode()
        assert text in msg, msg

    p = buf.data_ptr()
    refused("frames_planes: rgb24 frames hold no Y'CbCr planes", p, 180, 1, H, W, yr.LAYOUT_ID["rgb24"], 0, 8)
    refused("frames_planes: n must be 1 .. 16 (got 17)", p, 90, 17, H, W, L420, 0, 8)
    refused("frames_planes: unknown layout 3", p, 90, 1, H, W, 3, 0, 8)
    refused("frames_planes: depth must be 8 .. 16 (got 17)", p, 90, 1, H, W, L420, 0, 17)
    refused("frames_planes: unknown range 7", p, 90, 1, H, W, L420, 7, 8)
    refused("frames_planes: image size must be 1 .. 32768 (got 0 x 10)", p, 90, 1, 0, W, L444, 0, 8)
    refused("frames_planes: yuv420p needs even H and W (got 5 x 10)", p, 90, 1, 5, W, L420, 0, 8)
    refused("frames_planes: in_stride 89 is shorter than a frame (90 bytes)", p, 89, 2, H, W, L420, 0, 8)
    refused("frames_planes: the frame base is not 2-byte aligned", p + 1, 180, 1, H, W, L420, 0, 10)
    refused("frames_planes: in_stride 181 is not a multiple of 2", p, 181, 2, H, W, L420, 0, 12)
    assert _untouched(out)
    from gsvc_amd import yuv_loss
    from gsvc_amd.frames_out import FrameFormat
    with pytest.raises(ValueError, match="rgb24 frames hold no Y'CbCr planes"):
        yuv_loss.frame_planes(buf[:180], H, W, FrameFormat("rgb24"))
    with pytest.raises(ValueError, match="frames must be"):
        yuv_loss.frame_planes(buf[:89], H, W, FrameFormat("yuv420p"))
    # the wrapper, more than one launch (17 frames), against the entry point's own result
    codes = yr.make_codes(H, W, "yuv420p", 8, seed=5, n=17)
    got = yuv_loss.frame_planes(torch.from_numpy(codes).cuda(), H, W, FrameFormat("yuv420p", range="full"))
    want = np.stack([yr.code_planes_ref(c, H, W, "full", 8) for c in codes])
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


# ================================================================================================================ the transform, forward
def _forward(f, b, layout, matrix, shift=0, want_avg=True):
    lb, L, st = _lib()
    _, H, W = f.shape
    n = yr.plane_floats(H, W, layout)
    planes, avg = _sentinel(n, shift), (_sentinel(3 * H * W, shift) if want_avg else None)
    lb.check(L.gsvc_yuv_planes_forward(lb.ptr(f), lb.ptr(b), H, W, yr.LAYOUT_ID[layout], yr.MATRIX_ID[matrix], lb.ptr(planes), lb.ptr(avg), st),
             "gsvc_yuv_planes_forward")
    assert _written(planes, n) and (avg is None or _written(avg, 3 * H * W))
    return planes[:n], (avg[:3 * H * W].view(3, H, W) if avg is not None else None)


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
@pytest.mark.parametrize("layout,H,W", CASES, ids=CASE_IDS)
def test_planes_forward(layout, H, W, matrix, pair):
    f, b = _images(H, W, 100 + H + W, pair)
    planes, avg = _forward(f, b, layout, matrix)
    ref, _ = yr.planes_ref(f.double(), b.double() if pair else None, layout, matrix)
    p32, a32 = yr.planes_ref(f, b, layout, matrix)
    _rule(f"fwd {layout} {H}x{W} {matrix} pair={pair}", err(planes, ref, 1.0), err(p32, ref, 1.0))
    assert _same_bits(avg, a32)                       # 0.5 (f + flip(b)) is one rounding of its inputs; f itself without b
    again, avg2 = _forward(f, b, layout, matrix)
    assert _same_bits(planes, again) and _same_bits(avg, avg2)
    # the same bits on the other path (every base 4 bytes off 16-byte alignment), and without the averaged frame
    other, avg3 = _forward(_shifted(f), _shifted(b) if pair else None, layout, matrix, shift=1)
    assert _same_bits(planes, other) and _same_bits(avg, avg3)
    bare, none = _forward(f, b, layout, matrix, want_avg=False)
    assert none is None and _same_bits(planes, bare)


# ================================================================================================================ the transform, backward
def _backward(g, H, W, layout, matrix, pair, shift=0):
    lb, L, st = _lib()
    n = 3 * H * W
    d_f, d_b = _sentinel(n, shift), _sentinel(n, shift)
    lb.check(L.gsvc_yuv_planes_backward(lb.ptr(g), H, W, yr.LAYOUT_ID[layout], yr.MATRIX_ID[matrix], lb.ptr(d_f), lb.ptr(d_b) if pair else None, st),
             "gsvc_yuv_planes_backward")
    assert _written(d_f, n)
    if not pair:
        assert _untouched(d_b)                        # nothing is written that was not asked for
        return d_f[:n].view(3, H, W), None
    assert _written(d_b, n)
    return d_f[:n].view(3, H, W), d_b[:n].view(3, H, W)


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
@pytest.mark.parametrize("layout,H,W", CASES, ids=CASE_IDS)
def test_planes_backward_is_the_adjoint(layout, H, W, matrix, pair):
    gen = torch.Generator().manual_seed(300 + H + W)
    g = torch.randn(yr.plane_floats(H, W, layout), generator=gen).cuda()
    d_f, d_b = _backward(g, H, W, layout, matrix, pair)
    r_f, r_b = yr.adjoint_ref(g.double(), H, W, layout, matrix, pair)
    s_f, s_b = yr.adjoint_ref(g, H, W, layout, matrix, pair)
    scale = float(g.abs().max())
    tag = f"bwd {layout} {H}x{W} {matrix} pair={pair}"
    _rule(tag + " d_f", err(d_f, r_f, scale), err(s_f, r_f, scale))
    if pair:
        _rule(tag + " d_b", err(d_b, r_b, scale), err(s_b, r_b, scale))
    o_f, o_b = _backward(_shifted(g), H, W, layout, matrix, pair, shift=1)
    assert _same_bits(d_f, o_f) and (not pair or _same_bits(d_b, o_b))
    # <J x, y> = <x, J^T y> with both sides from the kernels, summed in float64; J x = planes(x) - planes(0) (the chroma's + 0.5).  The
    # gap is measured on the scale of the products, sum |J x| |y|, against the same gap of the fp32 tensor statements
    x_f, x_b = _images(H, W, 500 + H + W, pair)
    zero = torch.cat([torch.zeros(H * W), torch.full((yr.plane_floats(H, W, layout) - H * W,), 0.5)]).double().cuda()

    def gap(planes, df, db):
        jx = planes.double() - zero
        lhs = (jx * g.double()).sum()
        rhs = (x_f.double() * df.double()).sum() + ((x_b.double() * db.double()).sum() if pair else 0.0)
        return float((lhs - rhs).abs() / (jx.abs() * g.double().abs()).sum())
    planes, _ = _forward(x_f, x_b, layout, matrix)
    _rule(tag + " adjoint identity", gap(planes, d_f, d_b), gap(yr.planes_ref(x_f, x_b, layout, matrix)[0], s_f, s_b))


# ================================================================================================================ yuv_ssim_l1
@pytest.mark.parametrize("layout,H,W", CASES, ids=CASE_IDS)
def test_yuv_ssim_l1_value_and_gradients(layout, H, W):
    from gsvc_amd.frames_out import FrameFormat
    from gsvc_amd.yuv_loss import split_planes, yuv_planes, yuv_ssim_l1
    matrix = "bt601" if (H + W) % 4 == 0 else "bt709"
    f, b = _images(H, W, 700 + H + W, True)
    gt, _ = _images(H, W, 900 + H + W, False)
    with torch.no_grad():
        tY, tC, _ = yuv_planes((0.7 * gt + 0.3 * 0.5 * (f + b.flip(-1))).clamp(0, 1), None, layout, matrix)
    up = [0.3, -0.6, 0.2, -0.4]                       # the step's signs: SSIM terms enter negatively
    w = ssim_window()

    def combined(terms):
        return sum(c * t for c, t in zip(up, terms))

    def reference(dtype):
        ff, bb = f.detach().to(dtype).clone().requires_grad_(True), b.detach().to(dtype).clone().requires_grad_(True)
        terms = yr.yuv_ssim_l1_ref(ff, bb, tY.to(dtype), tC.to(dtype), layout, matrix, w)
        return [t.detach() for t in terms], torch.autograd.grad(combined(terms), (ff, bb))
    t64, g64 = reference(torch.float64)
    t32, g32 = reference(torch.float32)
    ff, bb = f.clone().requires_grad_(True), b.clone().requires_grad_(True)
    out = yuv_ssim_l1(ff, bb, (tY, tC), FrameFormat(layout, matrix))
    assert _same_bits(out[4], 0.5 * (f + b.flip(-1))) and not out[4].requires_grad
    combined(out[:4]).backward()
    tag = f"yuv_ssim_l1 {layout} {H}x{W}"
    for k, name in enumerate(("ssim_y", "l1_y", "ssim_c", "l1_c")):
        _rule(f"{tag} {name}", err(out[k].detach(), t64[k], 1.0), err(t32[k], t64[k], 1.0))
    for got, r64, r32, name in ((ff.grad, g64[0], g32[0], "d_f"), (bb.grad, g64[1], g32[1], "d_b")):
        scale = float(r64.abs().max())
        _rule(f"{tag} {name}", err(got, r64, scale), err(r32, r64, scale))
    Y, Cc = split_planes(torch.arange(yr.plane_floats(H, W, layout)), H, W, layout)
    assert tuple(Y.shape) == (1, H, W) and tuple(Cc.shape) == (2,) + yr.chroma_size(H, W, layout)


# ================================================================================================================ the step
H_, W_, T_ = 48, 64, 8


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """A yuv420p Y4M clip of the synthetic video, 8 frames of 64 x 48."""
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import FrameFormat, Y4MWriter, frames_to_u8
    path = str(tmp_path_factory.mktemp("yuv_loss") / "clip.y4m")
    cube = SyntheticFrameCube(H_, W_, T_, seed=7, device="cuda")
    fmt = FrameFormat("yuv420p")
    with Y4MWriter(path, W_, H_, (25, 1), fmt) as sink:
        for fr in frames_to_u8([cube._image(t) for t in range(T_)], fmt).cpu():
            sink.write(fr)
    return path


def _fit(path, domain, resident, steps=100, anchors=3000):
    from gsvc_amd.arguments import cfg_20240919
    from gsvc_amd.fit_setup import configure_fit, new_fit
    from gsvc_amd.frames_in import VideoFileCube
    cube = VideoFileCube(path, resident=resident)
    mp_, opt, pipe = cfg_20240919()
    opt.optical_lambda = 0.0
    configure_fit(mp_, opt, cube, steps, 0.004, 8.0, 2e-5)
    opt.loss_domain = domain
    pc, trainer = new_fit(cube, mp_, opt, pipe, anchors, torch.device("cuda", 0))
    return cube, opt, pc, trainer


def _distortion(out, cube, opt, fmt):
    """0.75 D_Y + 0.25 D_C of a step's two averaged frames against the file's planes, D = (1 - l) L1 + l (1 - SSIM), as a float."""
    from gsvc_amd.yuv_loss import target_planes, yuv_ssim_l1
    lam, total = opt.lambda_dssim, 0.0
    with torch.no_grad():
        for image, i in ((out.image1, out.frame_idx), (out.image2, out.frame_idx + 1)):
            sy, ly, sc, lc, _ = yuv_ssim_l1(image, None, target_planes(cube, i, fmt.layout, fmt.matrix), fmt)
            total += 0.75 * ((1 - lam) * float(ly) + lam * (1 - float(sy))) + 0.25 * ((1 - lam) * float(lc) + lam * (1 - float(sc)))
    return total


def test_step_loss_is_its_terms_and_is_deterministic(clip, monkeypatch):
    from gsvc_amd import switches
    from gsvc_amd.loss_utils import render_regs
    from gsvc_amd.yuv_loss import distortion_weights, target_planes, yuv_ssim_l1
    monkeypatch.setenv("GSVC_DETERMINISTIC", "1")
    switches.reload()
    losses = []
    for resident in ("u8", "u8", "float"):
        cube, opt, pc, trainer = _fit(clip, "yuv420", resident)
        assert trainer.loss_domain == "yuv420" and trainer.loss_matrix == "bt709" and trainer._distortion.native_planes
        out = trainer.step(1, frame_idx=2)
        torch.cuda.synchronize()
        losses.append(out.loss.clone())
        # by hand: the image terms from the step's own renders and the file's planes, the two regularisers from the step's batch
        fmt = trainer._distortion.fmt
        r1f, r1b, r2f, r2b = out.renders
        with torch.no_grad():
            y1 = yuv_ssim_l1(r1f.rendered_image, r1b.rendered_image, target_planes(cube, 2, fmt.layout, fmt.matrix), fmt)
            y2 = yuv_ssim_l1(r2f.rendered_image, r2b.rendered_image, target_planes(cube, 3, fmt.layout, fmt.matrix), fmt)
            batch = r1f.generated_gaussians.batch
            regs = render_regs(batch.scaling, batch.neural_opacity, batch.mask, batch.seg_offsets)
        assert not trainer.controller.entropy_constrained          # (step 1 is full precision: no rate term)
        weights, const = distortion_weights("yuv420", opt.lambda_dssim)
        terms = [y1[1], y2[1], y1[3], y2[3], y1[0], y2[0], y1[2], y2[2], regs[0], regs[1]]
        weights = weights + [opt.scaling_reg, opt.opacity_reg]
        prods = [wt * float(t.double()) for wt, t in zip(weights, terms)]
        by_hand = sum(prods) + const
        # the step forms the same sum as one fp32 dot product of ten terms plus a constant: at most eleven roundings of partial sums
        # that are no larger than the sum of the magnitudes
        bound = 16 * EPS32 * (sum(abs(v) for v in prods) + abs(const))
        if PRINT:
            print(f"YUV_STEP {resident}: loss {float(out.loss):.9g} by hand {by_hand:.9g} bound {bound:.3e}")
        assert abs(float(out.loss.double()) - by_hand) <= bound, (float(out.loss), by_hand, bound)
        assert _same_bits(out.image1, y1[4]) and _same_bits(out.image2, y2[4])
        trainer.close()
    assert np.isfinite(float(losses[0]))
    assert _same_bits(losses[0], losses[1]), "two equal starts"
    assert _same_bits(losses[0], losses[2]), "resident u8 against resident float"


def test_step_launches_no_conversion_nobody_reads(clip, monkeypatch):
    from gsvc_amd import frames_in
    calls = []
    real = frames_in.frames_from_u8

    def counted(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)
    monkeypatch.setattr(frames_in, "frames_from_u8", counted)
    cube, opt, pc, trainer = _fit(clip, "yuv420", "u8")
    assert not calls                                   # (resident="u8" keeps the bytes: the constructor converts nothing)
    for it in (1, 2, 3):
        trainer.step(it)
    torch.cuda.synchronize()
    trainer.close()
    assert not calls, f"{len(calls)} frames_from_u8 conversions in three yuv420 steps"
    cube, opt, pc, trainer = _fit(clip, "rgb", "u8")      # the counter counts: the rgb step reads converted pictures
    trainer.step(1)
    torch.cuda.synchronize()
    trainer.close()
    assert calls


def test_fit_in_the_yuv_domain_lowers_its_distortion(clip):
    """100 steps through the four phases per domain.  The yuv420 fit's own distortion (0.75 D_Y + 0.25 D_C on the file's planes) must
    fall between its first and its last ten steps; the rgb fit's is printed beside it and nothing is claimed about the pair."""
    from gsvc_amd.frames_out import FrameFormat
    fmt = FrameFormat("yuv420p")
    curves = {}
    for domain in ("yuv420", "rgb"):
        cube, opt, pc, trainer = _fit(clip, domain, "float")
        curve = []
        for it in range(1, 101):
            out = trainer.step(it)
            curve.append(_distortion(out, cube, opt, fmt))
        trainer.close()
        curves[domain] = curve
        assert all(np.isfinite(curve)), domain
    first, last = (float(np.mean(curves["yuv420"][:10])), float(np.mean(curves["yuv420"][-10:])))
    print(f"YUV_FIT yuv420: first ten {first:.5f} last ten {last:.5f}; rgb: first ten {np.mean(curves['rgb'][:10]):.5f} "
          f"last ten {np.mean(curves['rgb'][-10:]):.5f}")
    assert last < first, (first, last)


def test_domains_on_datasets_without_native_planes(clip, tmp_path):
    """Where a dataset has no planes of the requested layout the targets are the transform of its RGB pictures: a synthetic cube in
    both yuv domains, and a yuv444p file in the 4:2:0 domain (which hands out its own planes in the 4:4:4 domain)."""
    from gsvc_amd.arguments import cfg_20240919
    from gsvc_amd.fit_setup import configure_fit, new_fit
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_in import VideoFileCube
    from gsvc_amd.frames_out import FrameFormat, Y4MWriter, frames_to_u8
    from gsvc_amd.yuv_loss import split_planes, target_planes, yuv_planes
    synth = SyntheticFrameCube(H_, W_, T_, seed=7, device="cuda")
    fmt444 = FrameFormat("yuv444p", "bt601")
    path444 = str(tmp_path / "clip444.y4m")
    with Y4MWriter(path444, W_, H_, (25, 1), fmt444) as sink:
        for fr in frames_to_u8([synth._image(t) for t in range(T_)], fmt444).cpu():
            sink.write(fr)
    file444 = VideoFileCube(path444, fmt=fmt444, resident="u8")
    for cube, domain, native, matrix in ((synth.materialize(), "yuv420", False, "bt709"), (synth.materialize(), "yuv444", False, "bt709"),
                                         (file444, "yuv420", False, "bt601"), (file444, "yuv444", True, "bt601")):
        mp_, opt, pipe = cfg_20240919()
        opt.optical_lambda = 0.0
        configure_fit(mp_, opt, cube, 100, 0.004, 8.0, 2e-5)
        opt.loss_domain = domain
        pc, trainer = new_fit(cube, mp_, opt, pipe, 3000, torch.device("cuda", 0))
        assert (trainer._distortion.native_planes, trainer.loss_matrix) == (native, matrix)
        layout = trainer._distortion.fmt.layout
        tY, tC = target_planes(cube, 3, layout, matrix)
        if native:
            wY, wC = split_planes(cube.yuv_planes(3), H_, W_, layout)
        else:
            wY, wC, _ = yuv_planes(cube[3].image.permute(0, 2, 1).contiguous(), None, layout, matrix)
        assert _same_bits(tY, wY) and _same_bits(tC, wC)
        first = float(trainer.step(1, frame_idx=3).loss)
        for it in range(2, 21):
            last = float(trainer.step(it, frame_idx=3).loss)
        trainer.close()
        assert np.isfinite(first) and np.isfinite(last) and last < first, (domain, first, last)
    # the file's own 4:4:4 planes and the transform of its RGB pictures are the same picture where frames_from_u8 did not clamp: the
    # round trip codes -> R, G, B (three roundings of values below 1 each) -> planes (three more for Y, two for a chroma sample), with
    # six constants rounded to fp32 on either side, stays within about 8 eps32 of the plane; 16 eps32 is asked
    tY, tC = target_planes(file444, 3, "yuv444p", "bt601")
    wY, wC, _ = yuv_planes(file444[3].image.permute(0, 2, 1).contiguous(), None, "yuv444p", "bt601")
    in_gamut = (file444[3].image.permute(0, 2, 1) > 0).all(0) & (file444[3].image.permute(0, 2, 1) < 1).all(0)
    assert float(in_gamut.float().mean()) > 0.5
    assert float((tY - wY).abs()[0][in_gamut].max()) <= 16 * EPS32 and float((tC - wC).abs()[:, in_gamut].max()) <= 16 * EPS32


def test_encode_in_the_yuv_domain_then_decode_in_another_process(clip, tmp_path):
    """tools/gsvc_encode.py --loss-domain yuv420, then tools/gsvc_decode.py --strict in a fresh process: the loss domain changes the
    fit, not the file format."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gsvc_encode
    out, coded = str(tmp_path / "out.y4m"), str(tmp_path / "clip.gsvc")
    log = gsvc_encode.main([clip, "-o", coded, "--steps", "40", "--anchors", "2000", "--slab-frames", "8", "--densify-grad-threshold", "2e-5",
                            "--loss-domain", "yuv420"])
    assert log["loss_domain"] == "yuv420" and log["loss_matrix"] == "bt709" and log["total_bytes"] == os.path.getsize(coded)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gsvc_decode.py"), coded, "-o", out, "--strict"], cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-2500:])
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["frames_verified"] == T_ and line["frames_mismatched"] == 0
