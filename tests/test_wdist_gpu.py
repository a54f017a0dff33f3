"""GPU tests of the spatially weighted distortion: the kernels of csrc/wdist.hip through their C entry points
against the float64 run of their plain statements in tests/_wdist_ref.py, and the weights through the step, the encoder and its log.

Error rule (that of tests/test_loss_kernels_gpu.py): e_kernel <= 4 * e32 + 4 * eps32, both errors against the float64 reference on the
scale the case names, e32 being the error of the same reference function run in fp32 on the GPU on the same inputs (never the kernel's
own output).  Exact compares wherever an output is one fp32 rounding of its inputs or must be zero.  Output buffers are allocated longer
than needed and pre-filled with a NaN pattern no finite input produces: none may remain inside the range, all must survive past it.
GSVC_PRINT_ERRORS=1 prints e_kernel and e32 of every case.
"""
import os
import sys

import numpy as np
import pytest
import torch

from tests._loss_kernel_refs import EPS32, PRINT, err, ssim_l1_pair_ref, ssim_window
from tests._wdist_ref import (block_sse_ref, map_shape, pixel_weights, weighted_psnr_y_ref, wssim_l1_pair_ref, wssim_l1_ref,
                              wssim_partials)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SENTINEL = 0x7FC0BEEF            # a quiet NaN with a payload
PAD = 8


def _sentinel(n):
    return torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


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
        print(f"WDIST_ERR {tag}: kernel {e_k:.3e} fp32 statement {e32:.3e}")
    assert e_k <= 4 * e32 + 4 * EPS32, (tag, e_k, e32)


# ================================================================================================================ weighted SSIM / L1
CASES = [((3, 5, 7), 4), ((1, 32, 32), 8), ((3, 33, 65), 16), ((3, 37, 53), 4), ((2, 70, 100), 8)]
KINDS = ("rand", "rand_randn", "white", "flat")
WEIGHT_KINDS = ("ones", "rand", "rand_zeros")


def _images(kind, shape, seed):
    """Two images as tests/test_loss_kernels_gpu.py draws them, and the block of pixels on which they were forced equal."""
    Cc, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    if kind == "rand":
        a, b = torch.rand(shape, generator=gen), torch.rand(shape, generator=gen)
    elif kind == "rand_randn":
        a = torch.rand(shape, generator=gen)
        b = (a + 0.2 * torch.randn(shape, generator=gen)).clamp(0, 1)
    elif kind == "white":       # white background, the same textured patch at different offsets
        a, b = torch.ones(shape), torch.ones(shape)
        ph, pw = max(2, H // 2), max(2, W // 2)
        patch = torch.rand(Cc, ph, pw, generator=gen)
        a[:, 0:ph, 1:1 + pw] = patch
        b[:, H - ph:H, W - pw - 1:W - 1] = patch
    else:                       # flat bright
        a = (0.9 + 0.01 * torch.randn(shape, generator=gen)).clamp(0, 1)
        b = (a + 0.005 * torch.randn(shape, generator=gen)).clamp(0, 1)
    blk = (slice(None), slice(1, 4), slice(2, 6))
    a[blk] = b[blk]
    return a.cuda().contiguous(), b.cuda().contiguous(), blk


def _weights(kind, H, W, cell, seed):
    """[Hc, Wc] float32 on the device: all ones, uniform in [0.25, 4], or that with a third of the cells exactly 0."""
    Hc, Wc = map_shape(H, W, cell)
    gen = torch.Generator().manual_seed(seed)
    if kind == "ones":
        return torch.ones(Hc, Wc, device="cuda")
    w = 0.25 + 3.75 * torch.rand(Hc, Wc, generator=gen)
    if kind == "rand_zeros":
        n = Hc * Wc
        w.view(-1)[torch.randperm(n, generator=gen)[:(n + 2) // 3]] = 0.0
    return w.cuda().contiguous()


def _fwd(a, b, wts, cell, maps=True, pair_b=None):
    """(sums [2], maps or None, workspace, avg or None) of one forward call, every buffer guarded."""
    lb, L, st = _lib()
    Cc, H, W = a.shape
    n = a.numel()
    nw = int(L.gsvc_wssim_workspace_floats(Cc, H, W))
    assert nw == 2 * Cc * ((H + 31) // 32) * ((W + 31) // 32)
    sums, work = _sentinel(2), _sentinel(nw)
    m = [_sentinel(n) for _ in range(3)] if maps else [None] * 3
    avg = _sentinel(n) if pair_b is not None else None
    lb.check(L.gsvc_wssim_l1_forward(lb.ptr(a), lb.ptr(pair_b), lb.ptr(b), lb.ptr(wts), Cc, H, W, cell, lb.ptr(sums), lb.ptr(work),
                                     lb.ptr(m[0]), lb.ptr(m[1]), lb.ptr(m[2]), lb.ptr(avg), st), "gsvc_wssim_l1_forward")
    assert _written(sums, 2) and _written(work, nw) and all(_written(t, n) for t in m if t is not None)
    assert avg is None or _written(avg, n)
    return sums[:2], ([t[:n].view(a.shape) for t in m] if maps else None), work[:nw], (avg[:n].view(a.shape) if avg is not None else None)


def _bwd(a, b, wts, cell, maps, up, pair_b=None):
    lb, L, st = _lib()
    Cc, H, W = a.shape
    n = a.numel()
    grads = torch.tensor(up, dtype=torch.float32, device="cuda")
    d = _sentinel(n)
    db = _sentinel(n) if pair_b is not None else None
    lb.check(L.gsvc_wssim_l1_backward(lb.ptr(a), lb.ptr(pair_b), lb.ptr(b), lb.ptr(wts), Cc, H, W, cell, lb.ptr(grads), lb.ptr(maps[0]),
                                      lb.ptr(maps[1]), lb.ptr(maps[2]), lb.ptr(d), lb.ptr(db), st), "gsvc_wssim_l1_backward")
    assert _written(d, n) and (db is None or _written(db, n))
    if pair_b is None:
        return d[:n].view(a.shape)
    return d[:n].view(a.shape), db[:n].view(a.shape)


def _grad_ref(a, b, wts, cell, up, dtype):
    x = a.to(dtype).clone().requires_grad_(True)          # (a copy: .to() of the same dtype is the tensor itself)
    s, l1 = wssim_l1_ref(x, b.to(dtype), wts, cell, ssim_window())
    (d,) = torch.autograd.grad(up[0] * s + up[1] * l1, x)
    return s.detach(), l1.detach(), d


def _against_float64(tag, a, b, wts, cell, sums, maps, d, up):
    """Means on the scale of 1, the three weighted partial maps and dL/dimg1 each on its own maximum."""
    w = ssim_window()
    n = a.numel()
    s64, l64, d64 = _grad_ref(a, b, wts, cell, up, torch.float64)
    s32, l32, d32 = _grad_ref(a, b, wts, cell, up, torch.float32)
    _rule(f"{tag} ssim mean", abs(float(sums[0].double() / n) - float(s64)), abs(float(s32.double()) - float(s64)))
    _rule(f"{tag} l1 mean", abs(float(sums[1].double() / n) - float(l64)), abs(float(l32.double()) - float(l64)))
    p64, p32 = wssim_partials(a.double(), b.double(), wts, cell, w), wssim_partials(a, b, wts, cell, w)
    for k, nm in enumerate(("dm_dmu1", "dm_de11", "dm_de12")):
        sc = float(p64[k].abs().max())
        _rule(f"{tag} {nm}", err(maps[k], p64[k], sc), err(p32[k], p64[k], sc))
    sc = float(d64.abs().max())
    _rule(f"{tag} dL/dimg1", err(d, d64, sc), err(d32, d64, sc))


@pytest.mark.parametrize("shape,cell", CASES)
def test_wssim_l1_against_float64(shape, cell):
    """Every image kind and every weight kind (ones, uniform in [0.25, 4], a third of the cells exactly 0) at shapes with partial cells,
    several tiles and cells that span tile borders: means, the three weighted partial maps and the gradient for upstream (-0.2, 0.8) by
    the error rule.  Upstream (0, 1): exactly sign(x - y) * (fp32(1 / (C H W)) * w_pix), so exactly 0 on zero-weight cells and on the
    block where the images were forced equal; upstream (1, g) on that block: the SSIM part alone whatever g.  Sums and maps
    bit-identical between two runs and the sums with and without the maps.
    measured on the MI355X, largest over the five cases and three weight kinds, kernel / fp32 statement (each pair from the case where
    the kernel's error is largest):
      noise (both kinds)   ssim mean 1.3e-7 / 1.9e-8, l1 mean 2.2e-8 / 2.2e-8, maps 3.6e-6 / 3.6e-6 (dm_dmu1), dL/dimg1 4.0e-7 / 4.2e-7
      white background     ssim mean 6.7e-6 / 6.7e-6, l1 mean 2.2e-8 / 1.1e-8, maps 8.3e-4 / 9.2e-4 (dm_dmu1), dL/dimg1 2.9e-5 / 1.7e-5
      flat bright          ssim mean 5.5e-6 / 5.0e-6, l1 mean 5.6e-10 / 5.2e-10, maps 9.9e-3 / 1.1e-2 (dm_dmu1), dL/dimg1 1.1e-4 / 9.5e-5
    the figures of the unweighted kernels (tests/test_loss_kernels_gpu.py): the weights cost no accuracy."""
    Cc, H, W = shape
    inv = np.float32(1.0) / (np.float32(Cc) * np.float32(H) * np.float32(W))
    for i, kind in enumerate(KINDS):
        a, b, blk = _images(kind, shape, 100 * H + i)
        for j, wkind in enumerate(WEIGHT_KINDS):
            wts = _weights(wkind, H, W, cell, 10 * H + j)
            wp = pixel_weights(wts, cell, H, W)
            tag = f"wssim {shape}/{cell} {kind} {wkind}"
            sums, maps, _, _ = _fwd(a, b, wts, cell)
            d = _bwd(a, b, wts, cell, maps, (-0.2, 0.8))
            _against_float64(tag, a, b, wts, cell, sums, maps, d, (-0.2, 0.8))
            # the L1 subgradient, bit for bit
            d01 = _bwd(a, b, wts, cell, maps, (0.0, 1.0))
            assert torch.equal(d01, torch.sign(a - b) * (wp * float(inv)))
            assert not d01[blk].any() and bool((a[blk] == b[blk]).all())
            assert not d01[:, wp == 0].any()
            if wkind == "rand_zeros":
                assert bool((wp == 0).any()) and all(not m[:, wp == 0].any() for m in maps)          # "don't care": no map, no sum
            d10, d17 = _bwd(a, b, wts, cell, maps, (1.0, 0.0)), _bwd(a, b, wts, cell, maps, (1.0, 0.7))
            assert torch.equal(d10[blk], d17[blk])
            assert wkind != "ones" or bool(d10[blk].any())
            # the same bits without the maps and in a second run
            sums_nomaps = _fwd(a, b, wts, cell, maps=False)[0]
            sums_again, maps_again, _, _ = _fwd(a, b, wts, cell)
            assert torch.equal(sums, sums_nomaps) and torch.equal(sums, sums_again)
            assert all(torch.equal(p, q) for p, q in zip(maps, maps_again))


def test_wssim_l1_more_tiles_than_the_unweighted_kernel_has_slots():
    """(1, 1056, 1056) / 16: 33 x 33 = 1 089 tiles, more than the 1 024 slots of k_ssim_fwd's workspace: the workspace has a row per
    tile, every row is written, and the sums are the rows added in double (against their float64 sum: one fp32 rounding).  Random
    weights; means, maps and gradient by the error rule; two runs and the run without maps give the same bits.
    measured on the MI355X: ssim mean 1.2e-9 / 3.3e-10, l1 mean 7.7e-9 / 1.9e-8, maps 5.2e-6 / 4.8e-6 (dm_de11), dL/dimg1 3.9e-7 / 5.3e-7,
    rows 8.1e-8 / 9.6e-8."""
    shape, cell = (1, 1056, 1056), 16
    Cc, H, W = shape
    a, b, _ = _images("rand", shape, 1056)
    wts = _weights("rand", H, W, cell, 1056)
    sums, maps, work, _ = _fwd(a, b, wts, cell)
    assert work.numel() == 2 * 1089 and bool((work.view(1089, 2) != 0).all())
    d = _bwd(a, b, wts, cell, maps, (-0.2, 0.8))
    _against_float64(f"wssim {shape}/{cell} rand rand", a, b, wts, cell, sums, maps, d, (-0.2, 0.8))
    rows = work.view(1089, 2).double().sum(0)
    assert bool(((sums.double() - rows).abs() <= 2 * EPS32 * rows.abs()).all())
    # the rows themselves: row = bx + 33 by holds the weighted |x - y| sum of its tile
    wp = pixel_weights(wts, cell, H, W)

    def tiles(dtype):
        t = (wp.to(dtype) * (a.to(dtype) - b.to(dtype)).abs())[0]
        return t.view(33, 32, 33, 32).sum(dim=(1, 3)).reshape(-1)

    t64 = tiles(torch.float64)
    sc = float(t64.detach().max())
    _rule("wssim workspace: weighted l1 sums per tile", err(work.view(1089, 2)[:, 1], t64, sc), err(tiles(torch.float32), t64, sc))
    sums_nomaps = _fwd(a, b, wts, cell, maps=False)[0]
    sums_again, maps_again, work_again, _ = _fwd(a, b, wts, cell)
    assert torch.equal(sums, sums_nomaps) and torch.equal(sums, sums_again) and torch.equal(work, work_again)
    assert all(torch.equal(p, q) for p, q in zip(maps, maps_again))


@pytest.mark.parametrize("shape,cell", [((3, 33, 65), 8), ((3, 37, 53), 4)])
def test_wssim_l1_pair(shape, cell):
    """The pair form (odd W: the centre column maps onto itself): avg_out is (f + flip(b)) / 2 bit for bit; sums and maps are those of
    the single-image call on that average; value and both gradients by the rule against the float64 reference on the averaged image;
    dL_dimg_b is the flip of dL_dimg_f exactly, each half the single-image gradient.
    measured on the MI355X, larger of the two shapes: ssim mean 1.7e-8 / 5.8e-9, l1 mean 6.1e-9 / 1.7e-9, dL/df and dL/db 3.0e-7 / 2.8e-7."""
    Cc, H, W = shape
    gen = torch.Generator().manual_seed(7 * H + W)
    f, bk, gt = (torch.rand(shape, generator=gen).cuda() for _ in range(3))
    wts = _weights("rand_zeros", H, W, cell, H)
    sums, maps, _, avg = _fwd(f, gt, wts, cell, pair_b=bk)
    want_avg = (f + bk.flip(2)) / 2
    assert torch.equal(avg, want_avg)
    sums1, maps1, _, _ = _fwd(want_avg, gt, wts, cell)
    assert torch.equal(sums, sums1) and all(torch.equal(p, q) for p, q in zip(maps, maps1))
    up = (-0.2, 0.8)
    df, db = _bwd(f, gt, wts, cell, maps, up, pair_b=bk)
    d1 = _bwd(want_avg, gt, wts, cell, maps1, up)
    assert torch.equal(df, 0.5 * d1) and torch.equal(db, df.flip(2))
    if W % 2:
        assert torch.equal(db[:, :, W // 2], df[:, :, W // 2])
    w = ssim_window()
    outs = {}
    for dt in (torch.float64, torch.float32):
        fl, bl = f.to(dt).requires_grad_(True), bk.to(dt).requires_grad_(True)
        s, l1 = wssim_l1_pair_ref(fl, bl, gt.to(dt), wts, cell, w)
        outs[dt] = (s.detach(), l1.detach()) + torch.autograd.grad(up[0] * s + up[1] * l1, (fl, bl))
    s64, l64, f64, b64 = outs[torch.float64]
    s32, l32, f32_, b32 = outs[torch.float32]
    n = f.numel()
    _rule(f"wpair {shape} ssim mean", abs(float(sums[0].double() / n) - float(s64)), abs(float(s32.double()) - float(s64)))
    _rule(f"wpair {shape} l1 mean", abs(float(sums[1].double() / n) - float(l64)), abs(float(l32.double()) - float(l64)))
    sc = float(f64.abs().max())
    _rule(f"wpair {shape} dL/df", err(df, f64, sc), err(f32_, f64, sc))
    _rule(f"wpair {shape} dL/db", err(db, b64, sc), err(b32, b64, sc))


def test_wssim_l1_refusals_write_nothing():
    """NULL pointers, a cell outside {4, 8, 16}, one or two of the three maps, img1b without avg_out / dL_dimg1b: GsvcError, and no
    buffer is touched."""
    lb, L, st = _lib()
    shape, cell = (2, 20, 24), 8
    Cc, H, W = shape
    n = Cc * H * W
    a, b, _ = _images("rand", shape, 1)
    wts = _weights("rand", H, W, cell, 1)
    nw = int(L.gsvc_wssim_workspace_floats(Cc, H, W))
    sums, work, avg, d, db = _sentinel(2), _sentinel(nw), _sentinel(n), _sentinel(n), _sentinel(n)
    m = [_sentinel(n) for _ in range(3)]
    grads = torch.ones(2, device="cuda")
    P = lb.ptr

    def fwd(img1=a, img1b=None, img2=b, w=wts, c=cell, s=sums, ws=work, maps=(None, None, None), av=None):
        lb.check(L.gsvc_wssim_l1_forward(P(img1), P(img1b), P(img2), P(w), Cc, H, W, c, P(s), P(ws), P(maps[0]), P(maps[1]), P(maps[2]),
                                         P(av), st), "gsvc_wssim_l1_forward")

    def bwd(img1=a, img1b=None, img2=b, w=wts, c=cell, g=grads, maps=tuple(m), out=d, outb=None):
        lb.check(L.gsvc_wssim_l1_backward(P(img1), P(img1b), P(img2), P(w), Cc, H, W, c, P(g), P(maps[0]), P(maps[1]), P(maps[2]), P(out),
                                          P(outb), st), "gsvc_wssim_l1_backward")

    for kw in (dict(img1=None), dict(img2=None), dict(w=None), dict(s=None), dict(ws=None)):
        with pytest.raises(lb.GsvcError, match="wssim_l1_forward: NULL pointer"):
            fwd(**kw)
    for kw in (dict(img1=None), dict(img2=None), dict(w=None), dict(g=None), dict(out=None), dict(maps=(None, m[1], m[2])), dict(maps=(m[0], m[1], None))):
        with pytest.raises(lb.GsvcError, match="wssim_l1_backward: NULL pointer"):
            bwd(**kw)
    for c in (0, 2, 5, 12, 32, -8):
        with pytest.raises(lb.GsvcError, match="cell must be 4, 8 or 16"):
            fwd(c=c)
        with pytest.raises(lb.GsvcError, match="cell must be 4, 8 or 16"):
            bwd(c=c)
    for maps in ((m[0], None, None), (m[0], m[1], None), (None, m[1], None), (None, None, m[2])):
        with pytest.raises(lb.GsvcError, match="pass all three partial maps or none"):
            fwd(maps=maps)
    with pytest.raises(lb.GsvcError, match="the pair form needs avg_out"):
        fwd(img1b=a, maps=tuple(m))
    with pytest.raises(lb.GsvcError, match="needs img1b and dL_dimg1b together"):
        bwd(img1b=a)
    assert int(L.gsvc_wssim_workspace_floats(0, H, W)) == -1 and int(L.gsvc_wssim_workspace_floats(Cc, H, -1)) == -1
    torch.cuda.synchronize()
    assert all(_untouched(t) for t in [sums, work, avg, d, db] + m)


# ================================================================================================================ per-cell luma SSE
def _codes(n, H, W, layout, depth, seed, pad=0):
    """Random frames uint8 [n, frame bytes + pad] on the device (deep: little-endian 16-bit samples below 2^depth)."""
    from gsvc_amd.frames_out import FrameFormat, frame_bytes
    fmt = FrameFormat(layout, depth=depth)
    nbytes = frame_bytes(H, W, fmt)
    rng = np.random.default_rng(seed)
    buf = np.zeros((n, nbytes + pad), dtype=np.uint8)
    if depth > 8:
        buf[:, :nbytes] = rng.integers(0, 1 << depth, (n, nbytes // 2)).astype("<u2").view(np.uint8)
    else:
        buf[:, :nbytes] = rng.integers(0, 256, (n, nbytes))
    return fmt, nbytes, torch.from_numpy(buf).cuda()


@pytest.mark.parametrize("layout", ["yuv420p", "yuv444p"])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("H,W", [(18, 22), (40, 36)])
def test_block_sse_equals_the_reference(H, W, depth, layout):
    """n = 3 frames at 18 x 22 (W no multiple of 4: one sample per load) and 40 x 36 (one load per block row), cells 4 / 8 / 16, packed
    rows and rows 8 bytes apart: exactly the numpy sums, whose total per frame is ``plane_sse``'s luma entry; the output is written to
    its end and not past it."""
    from gsvc_amd.frames_out import LAYOUTS
    from gsvc_amd.metrics import plane_sse
    from gsvc_amd.wdist import block_sse
    lb, L, st = _lib()
    for pad in (0, 8):
        fmt, nbytes, a = _codes(3, H, W, layout, depth, 1 + pad, pad)
        _, _, b = _codes(3, H, W, layout, depth, 2 + pad, pad)
        luma = plane_sse(a, b, H, W, fmt)[:, 0]
        for cell in (4, 8, 16):
            got = block_sse(a, b, H, W, fmt, cell)
            want = block_sse_ref(a.cpu().numpy(), b.cpu().numpy(), H, W, depth, cell)
            assert got.dtype == torch.int64 and tuple(got.shape) == (3,) + map_shape(H, W, cell)
            assert np.array_equal(got.cpu().numpy(), want)
            assert torch.equal(got.sum(dim=(1, 2)), luma)
            cells = 3 * want.shape[1] * want.shape[2]
            out = torch.full((cells + PAD,), SENTINEL, dtype=torch.int64, device="cuda")
            lb.check(L.gsvc_frames_block_sse(a.data_ptr(), b.data_ptr(), nbytes + pad, 3, H, W, LAYOUTS[layout], depth, cell, out.data_ptr(), st),
                     "gsvc_frames_block_sse")
            assert np.array_equal(out[:cells].cpu().numpy().reshape(want.shape), want) and bool((out[cells:] == SENTINEL).all())


def test_block_sse_width_of_the_sums_and_refusals():
    """Two 16-bit frames that differ by 65 535 everywhere: every cell holds n_pix * 65535^2 (a full 16 x 16 cell: 1.1e12, far past 32
    bits).  A bad cell, rgb24 frames, NULL pointers and a short stride are refused with nothing written."""
    from gsvc_amd.frames_out import LAYOUTS, FrameFormat, frame_bytes
    from gsvc_amd.wdist import block_sse
    from tests._wdist_ref import pixels_of_cells
    lb, L, st = _lib()
    H, W = 40, 36
    fmt = FrameFormat("yuv420p", depth=16)
    nbytes = frame_bytes(H, W, fmt)
    a = torch.zeros((1, nbytes), dtype=torch.uint8, device="cuda")
    b = torch.full((1, nbytes), 255, dtype=torch.uint8, device="cuda")
    for cell in (4, 8, 16):
        want = (pixels_of_cells(H, W, cell).astype(np.int64) * 65535 ** 2)[None]
        assert np.array_equal(block_sse(a, b, H, W, fmt, cell).cpu().numpy(), want)
        assert np.array_equal(block_sse(b, a, H, W, fmt, cell).cpu().numpy(), want)
    assert int(want.max()) == 256 * 65535 ** 2 > 2 ** 32
    with pytest.raises(ValueError, match="cell must be one of"):
        block_sse(a, b, H, W, fmt, 5)
    with pytest.raises(ValueError, match="rgb24"):
        block_sse(a, b, H, W, FrameFormat("rgb24"), 8)
    out = torch.full((64,), SENTINEL, dtype=torch.int64, device="cuda")
    y = LAYOUTS["yuv420p"]
    for args, text in (((0, b.data_ptr(), nbytes, 1, H, W, y, 16, 8), "NULL pointer"),
                       ((a.data_ptr(), b.data_ptr(), nbytes, 1, H, W, y, 16, 12), "cell must be 4, 8 or 16"),
                       ((a.data_ptr(), b.data_ptr(), nbytes - 2, 1, H, W, y, 16, 8), "shorter than a frame"),
                       ((a.data_ptr(), b.data_ptr(), nbytes, 1, H, W, LAYOUTS["rgb24"], 8, 8), "no luma plane")):
        with pytest.raises(lb.GsvcError, match=text):
            lb.check(L.gsvc_frames_block_sse(*args, out.data_ptr(), st), "gsvc_frames_block_sse")
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ================================================================================================================ the step
H_, W_, T_ = 48, 64, 8
CELL_ = 8


def _fit(cube, steps=40, anchors=3000, **weighting):
    from gsvc_amd.arguments import cfg_20240919
    from gsvc_amd.fit_setup import configure_fit, new_fit
    mp_, opt, pipe = cfg_20240919()
    opt.optical_lambda = 0.0
    configure_fit(mp_, opt, cube, steps, 0.004, 8.0, 2e-5)
    pc, trainer = new_fit(cube, mp_, opt, pipe, anchors, torch.device("cuda", 0), **weighting)
    return opt, pc, trainer


def _cube():
    from gsvc_amd.frame import SyntheticFrameCube
    return SyntheticFrameCube(H_, W_, T_, seed=1234, device=torch.device("cuda", 0)).materialize()


def test_step_distortion_with_all_ones_maps_is_the_unweighted_distortion():
    """On the renders of one step of a tiny synthetic cube: ``StepDistortion`` with all-ones maps and the unweighted one each give the
    float64 pair reference's terms and gradients by the error rule (all-ones weights leave the definition unchanged; the two kernels
    add in different orders, so the bits may differ).
    measured on the MI355X, both objects alike: ssim 7.2e-8 / 4.3e-8, l1 1.4e-9 / 1.4e-9, dL/df and dL/db 8.9e-6 / 5.3e-6."""
    from gsvc_amd.loss_utils import StepDistortion
    cube = _cube()
    opt, pc, trainer = _fit(cube)
    out = trainer.step(1, frame_idx=3)
    torch.cuda.synchronize()
    ones = torch.ones((T_,) + map_shape(H_, W_, CELL_), device="cuda")
    plain, weighted = StepDistortion(opt, cube), StepDistortion(opt, cube, weight_maps=ones, weight_cell=CELL_)
    assert plain.weight_maps is None and weighted.weight_cell == CELL_
    w, up = ssim_window(), (-0.2, 0.8)
    for k, i in ((0, 3), (2, 4)):
        f, b = out.renders[k].rendered_image.detach().clone(), out.renders[k + 1].rendered_image.detach().clone()
        gt = plain.target(cube, cube[i], i, f.device)
        ref = {}
        for dt in (torch.float64, torch.float32):
            fl, bl = f.to(dt).requires_grad_(True), b.to(dt).requires_grad_(True)
            s, l1 = ssim_l1_pair_ref(fl, bl, gt.to(dt), w)
            ref[dt] = (s.detach(), l1.detach()) + torch.autograd.grad(up[0] * s + up[1] * l1, (fl, bl))
        s64, l64, f64, b64 = ref[torch.float64]
        s32, l32, f32_, b32 = ref[torch.float32]
        sc = float(f64.abs().max())
        for name, dist in (("plain", plain), ("ones", weighted)):
            fl, bl = f.clone().requires_grad_(True), b.clone().requires_grad_(True)
            (l1, s), image = dist(fl, bl, gt, frame_index=i)
            df, db = torch.autograd.grad(up[0] * s + up[1] * l1, (fl, bl))
            _rule(f"step {name} frame {i} ssim", abs(float(s.detach().double()) - float(s64)), abs(float(s32.double()) - float(s64)))
            _rule(f"step {name} frame {i} l1", abs(float(l1.detach().double()) - float(l64)), abs(float(l32.double()) - float(l64)))
            _rule(f"step {name} frame {i} dL/df", err(df, f64, sc), err(f32_, f64, sc))
            _rule(f"step {name} frame {i} dL/db", err(db, b64, sc), err(b32, b64, sc))
            assert torch.equal(image, (f + b.flip(2)) / 2)
    with pytest.raises(ValueError, match="needs frame_index"):
        weighted(f, b, gt)
    trainer.close()


def test_trainer_with_roi_maps_is_deterministic(monkeypatch):
    """Three steps with a region of interest under GSVC_DETERMINISTIC=1, twice from the same seed: the losses are the same bits (the
    weighted kernels have no atomics: the mode needs nothing extra), every parameter gradient that arrives is finite, and the maps are
    those of ``roi_weights`` on the model's device."""
    from gsvc_amd import switches, wdist
    rects = [(16, 12, 32, 24, 4.0), (0, 0, 8, 8, 0.0)]
    monkeypatch.setenv("GSVC_DETERMINISTIC", "1")
    switches.reload()
    try:
        runs = []
        for _ in range(2):
            opt, pc, trainer = _fit(_cube(), roi=rects, weight_cell=CELL_)
            assert trainer.weight_maps.is_cuda and trainer.weight_cell == CELL_ and trainer.weighting["sources"] == ["roi"]
            assert torch.equal(trainer.weight_maps.cpu(), wdist.roi_weights(H_, W_, CELL_, rects, T_))
            assert float(trainer.weight_maps.min()) == 0.0
            bad, seen = [], [0]

            def hook(name):
                def check(g):
                    seen[0] += 1
                    if not bool(torch.isfinite(g).all()):
                        bad.append(name)
                return check
            for name, p in pc.named_parameters():
                if p.requires_grad:
                    p.register_hook(hook(name))
            losses = [trainer.step(it, frame_idx=2 + it).loss.detach().clone() for it in (1, 2, 3)]
            torch.cuda.synchronize()
            assert seen[0] > 0 and not bad, bad
            assert all(bool(torch.isfinite(p).all()) for p in pc.parameters())
            trainer.close()
            runs.append(torch.stack(losses))
        assert bool(torch.isfinite(runs[0]).all())
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    finally:
        monkeypatch.delenv("GSVC_DETERMINISTIC", raising=False)
        switches.reload()
    # the weights change the fit: the same steps without them give another loss
    opt, pc, trainer = _fit(_cube())
    assert trainer.weight_maps is None and trainer.weighting is None
    plain = trainer.step(1, frame_idx=3).loss.detach().clone()
    trainer.close()
    assert float(plain) != float(runs[0][0])


# ================================================================================================================ the encoder
FIT = dict(steps=40, anchors=2000, slab_frames=8.0, densify_grad_threshold=2e-5)
OLD_LOG = {"W", "H", "frames", "steps", "init", "anchors_initial", "loss_domain", "loss_matrix", "distortion", "anchors_coded", "fit_seconds",
           "hash_format", "verify_decode_fps", "sections"}
OLD_SECTIONS = {"HEAD", "MLPS", "ANCH", "MASK", "HASH", "SLAB", "PHSH"}
EH, EW, ET = 64, 96, 8


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """The clip of the codec tests: 8 frames of 96 x 64 yuv420p of the synthetic video with a little noise -> {"path", "frames", "tmp"}."""
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import FrameFormat, Y4MWriter, frames_to_u8
    fmt = FrameFormat("yuv420p")
    tmp = tmp_path_factory.mktemp("wdist")
    cube = SyntheticFrameCube(EH, EW, ET, seed=7, device="cuda")
    clean = frames_to_u8([cube._image(t) for t in range(ET)], fmt).cpu().numpy().copy()
    del cube
    noisy = np.clip(np.rint(clean + np.random.default_rng(3).normal(0.0, 2.0, clean.shape)), 0, 255).astype(np.uint8)
    path = str(tmp / "clip.y4m")
    with Y4MWriter(path, EW, EH, (25, 1), fmt) as sink:
        for fr in noisy:
            sink.write(torch.from_numpy(fr))
    return {"path": path, "frames": noisy, "tmp": tmp}


class _Collect:
    """A sink that keeps its frames."""

    def __init__(self):
        self.rows = []

    def write(self, frame_u8):
        self.rows.append(np.array(frame_u8, copy=True).reshape(-1))

    def close(self):
        pass


def test_encode_gop_with_activity_weighting(clip):
    """``encode_gop(weighting="activity")``: the file decodes --strict and has the default sections (nothing of the weights is
    signalled); the log is the default key set plus "weighting"; its wpsnr_y and psnr_y are ``weighted_psnr_y`` of the decoded frames
    against the source under the maps ``activity_weights`` gives for the clip, recomputed here in numpy."""
    from gsvc_amd import bitstream as B
    from gsvc_amd import wdist
    from gsvc_amd.detail import cube_detail
    from gsvc_amd.fit_setup import encode_gop
    from gsvc_amd.frames_in import VideoFileCube
    from gsvc_amd.frames_out import FrameFormat
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gsvc_decode
    dev = torch.device("cuda", 0)
    blob, log = encode_gop(clip["path"], dev, weighting="activity", weight_strength=0.75, weight_cell=CELL_, **FIT)
    assert set(log) == OLD_LOG | {"weighting"} and set(log["sections"]) == OLD_SECTIONS
    wl = log["weighting"]
    assert set(wl) == {"sources", "cell", "strength", "clamp", "min", "max", "psnr_y", "wpsnr_y"}
    assert wl["sources"] == ["activity"] and wl["cell"] == CELL_ and wl["strength"] == 0.75 and 0 < wl["min"] < 1 < wl["max"]
    coded = str(clip["tmp"] / "activity.gsvc")
    with open(coded, "wb") as f:
        f.write(blob)
    assert gsvc_decode.main([coded, "-o", str(clip["tmp"] / "activity.y4m"), "--strict"]) == 0
    fmt = FrameFormat("yuv420p")
    sink = _Collect()
    res = B.decode_video(B.parse_bitstream(blob), sink, fmt=fmt, strict=True)
    assert res["verified"] and res["frames_verified"] == ET
    decoded = np.stack(sink.rows)
    cube = VideoFileCube(clip["path"], device=dev)
    maps = wdist.activity_weights(cube_detail(cube, CELL_), EH, EW, CELL_, 8, strength=0.75)
    del cube
    assert wl["min"] == float(maps.min()) and wl["max"] == float(maps.max())
    sse = block_sse_ref(decoded, clip["frames"], EH, EW, 8, CELL_)
    _, want_w = weighted_psnr_y_ref(sse, maps.numpy(), 8, EH, EW)
    _, want_p = weighted_psnr_y_ref(sse, np.ones(sse.shape), 8, EH, EW)
    print("weighting:", wl)
    assert abs(wl["wpsnr_y"] - want_w) < 1e-9 and abs(wl["psnr_y"] - want_p) < 1e-9 and wl["wpsnr_y"] != wl["psnr_y"]
    assert 10.0 < wl["psnr_y"] < 60.0


def test_encode_gop_without_the_arguments_has_the_default_log(clip):
    from gsvc_amd.fit_setup import encode_gop
    blob, log = encode_gop(clip["path"], torch.device("cuda", 0), **FIT)
    assert set(log) == OLD_LOG and set(log["sections"]) == OLD_SECTIONS
    with pytest.raises(ValueError, match="loss_domain must be 'rgb'"):
        encode_gop(clip["path"], torch.device("cuda", 0), roi=[(0, 0, 16, 16, 2.0)], loss_domain="yuv420", **FIT)
