"""The kernels that produce the loss value and the first gradients of every fitting step, called through their C entry points:
csrc/ssim.hip (fused SSIM + L1, single image and two-view pair), csrc/losses.hip (regularisers, optical-flow pair loss, single pair
and batched), csrc/rate.hip (k_rate_fwd / k_rate_bwd) and the noise quantiser of csrc/quant.hip, each against the float64 run of its
plain tensor statement in tests/_loss_kernel_refs.py.

Error rule: e_kernel <= 4 * e32 + 4 * eps32, both errors against the float64 reference on the scale the case names, e32 being the
error of the same reference function run in fp32 on the GPU on the same inputs (never the kernel's own output).  Exact compares
wherever an output is one fp32 rounding of its inputs or must be zero.  Output buffers are allocated longer than needed and
pre-filled with a NaN pattern no finite input produces: none may remain inside the range, all must survive past it.
GSVC_PRINT_ERRORS=1 prints e_kernel and e32 of every case.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests._loss_kernel_refs import (EPS32, LOW_BOUND, PRINT, err, err_each, noise_quant_grads, noise_quant_ref, optical_pair_ref,
                                     rate_bits_ref, regs_ref, ssim_l1_pair_ref, ssim_l1_ref, ssim_partials, ssim_window)

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF            # a quiet NaN with a payload
PAD = 8


def _sentinel(n):
    return torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _sentinel_i32(n):
    return torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")


def _written(buf, n):
    """Every element of [0, n) was written, none past n."""
    bits = buf.view(torch.int32)
    return bool((bits[:n] != SENTINEL).all()) and bool((bits[n:] == SENTINEL).all())


def _untouched(buf):
    return bool((buf.view(torch.int32) == SENTINEL).all())


def _zeros_guarded(n):
    """n zeros followed by the sentinel (for buffers the kernel adds to)."""
    b = _sentinel(n)
    b[:n] = 0
    return b


def _lib():
    from gsvc_amd import _lib
    return _lib, _lib.lib(), _lib.current_stream()


def _rule(tag, e_k, e32):
    if PRINT:
        print(f"LOSS_ERR {tag}: kernel {e_k:.3e} fp32 statement {e32:.3e}")
    assert e_k <= 4 * e32 + 4 * EPS32, (tag, e_k, e32)


def _i64(values):
    return (C.c_int64 * len(values))(*[int(v) for v in values])


def _i32(values):
    return (C.c_int32 * len(values))(*[int(v) for v in values])


def _f32(v):
    return float(np.float32(v))


# ================================================================================================================ SSIM / L1
SS_SLOTS = 1024
SSIM_SHAPES = [(3, 5, 7), (1, 32, 32), (3, 33, 65), (3, 37, 53), (2, 70, 100)]
SSIM_KINDS = ("rand", "rand_randn", "white", "flat")


def _ssim_inputs(kind, shape, seed):
    """Two images, and the block of pixels on which they were forced equal."""
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


def _ssim_fwd(a, b, maps=True, pair_b=None):
    """Returns (sums [2], maps or None, workspace, avg or None) of one forward call, with every buffer guarded."""
    lb, L, st = _lib()
    Cc, H, W = a.shape
    n = a.numel()
    sums, work = _sentinel(2), _sentinel(2 * SS_SLOTS)
    m = [_sentinel(n) for _ in range(3)] if maps else [None] * 3
    avg = None
    if pair_b is None:
        lb.check(L.gsvc_ssim_l1_forward(lb.ptr(a), lb.ptr(b), Cc, H, W, lb.ptr(sums), lb.ptr(work), lb.ptr(m[0]), lb.ptr(m[1]),
                                        lb.ptr(m[2]), st), "gsvc_ssim_l1_forward")
    else:
        avg = _sentinel(n)
        lb.check(L.gsvc_ssim_l1_pair_forward(lb.ptr(a), lb.ptr(pair_b), lb.ptr(b), Cc, H, W, lb.ptr(sums), lb.ptr(work), lb.ptr(m[0]),
                                             lb.ptr(m[1]), lb.ptr(m[2]), lb.ptr(avg), st), "gsvc_ssim_l1_pair_forward")
        assert _written(avg, n)
    assert _written(sums, 2) and _written(work, 2 * SS_SLOTS) and all(_written(t, n) for t in m if t is not None)
    return sums[:2], ([t[:n].view(a.shape) for t in m] if maps else None), work[:2 * SS_SLOTS], (avg[:n].view(a.shape) if avg is not None else None)


def _ssim_bwd(a, b, maps, up, pair_b=None):
    lb, L, st = _lib()
    Cc, H, W = a.shape
    n = a.numel()
    grads = torch.tensor(up, dtype=torch.float32, device="cuda")
    d = _sentinel(n)
    if pair_b is None:
        lb.check(L.gsvc_ssim_l1_backward(lb.ptr(a), lb.ptr(b), Cc, H, W, lb.ptr(grads), lb.ptr(maps[0]), lb.ptr(maps[1]), lb.ptr(maps[2]),
                                         lb.ptr(d), st), "gsvc_ssim_l1_backward")
        assert _written(d, n)
        return d[:n].view(a.shape)
    db = _sentinel(n)
    lb.check(L.gsvc_ssim_l1_pair_backward(lb.ptr(a), lb.ptr(pair_b), lb.ptr(b), Cc, H, W, lb.ptr(grads), lb.ptr(maps[0]), lb.ptr(maps[1]),
                                          lb.ptr(maps[2]), lb.ptr(d), lb.ptr(db), st), "gsvc_ssim_l1_pair_backward")
    assert _written(d, n) and _written(db, n)
    return d[:n].view(a.shape), db[:n].view(a.shape)


def _ssim_grad_ref(a, b, w, up, dtype):
    x = a.to(dtype).requires_grad_(True)
    s, l1 = ssim_l1_ref(x, b.to(dtype), w)
    (d,) = torch.autograd.grad(up[0] * s + up[1] * l1, x)
    return s.detach(), l1.detach(), d


def _ssim_against_float64(tag, a, b, sums, maps, d, up):
    """Means on the scale of 1, the three partial maps and dL/dimg1 each on its own maximum."""
    w = ssim_window()
    n = a.numel()
    s64, l64, d64 = _ssim_grad_ref(a, b, w, up, torch.float64)
    s32, l32, d32 = _ssim_grad_ref(a, b, w, up, torch.float32)
    _rule(f"{tag} ssim mean", abs(float(sums[0].double() / n) - float(s64)), abs(float(s32.double()) - float(s64)))
    _rule(f"{tag} l1 mean", abs(float(sums[1].double() / n) - float(l64)), abs(float(l32.double()) - float(l64)))
    p64, p32 = ssim_partials(a.double(), b.double(), w), ssim_partials(a, b, w)
    for k, nm in enumerate(("dm_dmu1", "dm_de11", "dm_de12")):
        sc = float(p64[k].abs().max())
        _rule(f"{tag} {nm}", err(maps[k], p64[k], sc), err(p32[k], p64[k], sc))
    sc = float(d64.abs().max())
    _rule(f"{tag} dL/dimg1", err(d, d64, sc), err(d32, d64, sc))


@pytest.mark.parametrize("shape", SSIM_SHAPES)
def test_ssim_l1_against_float64(shape):
    """Every input kind at every shape with at most 1024 blocks: means, partial maps and the gradient for upstream (-0.2, 0.8) by the
    error rule; upstream (0, 1): exactly fp32(1 / (C H W)) * sign(x - y), exactly 0 on the block where the images were forced equal;
    upstream (1, g) on that block: the SSIM part alone whatever g; sums bit-identical with and without the partial maps and between
    two runs; one or two maps are refused.
    measured on the MI355X, largest over the five shapes, kernel / fp32 statement:
      noise (both kinds)   ssim mean 7.6e-8 / 1.2e-7, l1 mean 3.0e-8 / 1.7e-8, maps 5.3e-6 / 4.5e-6, dL/dimg1 5.1e-7 / 5.6e-7
      white background     ssim mean 3.8e-6 / 3.8e-6, l1 mean 1.4e-8 / 1.3e-8, maps 8.3e-4 / 9.2e-4 (dm_dmu1), dL/dimg1 2.7e-5 / 2.6e-5
      flat bright          ssim mean 2.9e-6 / 1.9e-6, l1 mean 2.6e-10 / 4.2e-10, maps 9.9e-3 / 1.1e-2 (dm_dmu1), dL/dimg1 1.3e-4 / 1.1e-4
    so on the inputs where sigma^2 = E[x^2] - mu^2 cancels the kernel is as good as the formulation it replaced, no better."""
    lb, L, st = _lib()
    Cc, H, W = shape
    n = Cc * H * W
    inv = np.float32(1.0) / (np.float32(Cc) * np.float32(H) * np.float32(W))
    for i, kind in enumerate(SSIM_KINDS):
        a, b, blk = _ssim_inputs(kind, shape, 100 * H + i)
        tag = f"ssim {shape} {kind}"
        sums, maps, _, _ = _ssim_fwd(a, b)
        d = _ssim_bwd(a, b, maps, (-0.2, 0.8))
        _ssim_against_float64(tag, a, b, sums, maps, d, (-0.2, 0.8))
        # the L1 subgradient
        d01 = _ssim_bwd(a, b, maps, (0.0, 1.0))
        assert torch.equal(d01, torch.sign(a - b) * float(inv))
        assert not d01[blk].any() and bool((a[blk] == b[blk]).all())
        d10, d17 = _ssim_bwd(a, b, maps, (1.0, 0.0)), _ssim_bwd(a, b, maps, (1.0, 0.7))
        assert torch.equal(d10[blk], d17[blk]) and bool(d10[blk].any())
        _, _, d64 = _ssim_grad_ref(a, b, ssim_window(), (1.0, 0.0), torch.float64)
        _, _, d32 = _ssim_grad_ref(a, b, ssim_window(), (1.0, 0.0), torch.float32)
        sc = float(d64.abs().max())
        _rule(f"{tag} dL/dimg1 (1, 0)", err(d10, d64, sc), err(d32, d64, sc))
        # the same bits without the maps and in a second run
        sums_nomaps = _ssim_fwd(a, b, maps=False)[0]
        sums_again, maps_again, _, _ = _ssim_fwd(a, b)
        assert torch.equal(sums, sums_nomaps) and torch.equal(sums, sums_again)
        assert all(torch.equal(p, q) for p, q in zip(maps, maps_again))
    # one or two maps: refused, nothing launched
    sums, work, m0, m1 = _sentinel(2), _sentinel(2 * SS_SLOTS), _sentinel(n), _sentinel(n)
    for m in ((m0, None, None), (m0, m1, None), (None, m1, None), (None, None, m0)):
        with pytest.raises(lb.GsvcError, match="pass all three partial maps or none"):
            lb.check(L.gsvc_ssim_l1_forward(lb.ptr(a), lb.ptr(b), Cc, H, W, lb.ptr(sums), lb.ptr(work), lb.ptr(m[0]), lb.ptr(m[1]),
                                            lb.ptr(m[2]), st), "gsvc_ssim_l1_forward")
    torch.cuda.synchronize()
    assert _untouched(sums) and _untouched(m0) and _untouched(m1)


def test_ssim_l1_more_blocks_than_slots():
    """3 x 577 x 577: 19 x 19 x 3 = 1083 blocks fold into 1024 slots by modulo, so 59 slots receive two atomic adds.  Means, maps and
    gradient by the error rule, and the workspace itself: slot s holds the |x - y| sums of the tiles s and s + 1024, against the
    float64 tile sums on the scale of the largest.
    measured on the MI355X: slots 1.07e-7 / 1.09e-7; means, maps and gradient within the noise figures of the test above."""
    shape = (3, 577, 577)
    Cc, H, W = shape
    a, b, _ = _ssim_inputs("rand", shape, 577)
    sums, maps, work, _ = _ssim_fwd(a, b)
    d = _ssim_bwd(a, b, maps, (-0.2, 0.8))
    _ssim_against_float64(f"ssim {shape} rand", a, b, sums, maps, d, (-0.2, 0.8))
    gy, gx = (H + 31) // 32, (W + 31) // 32
    assert gx * gy * Cc == 1083

    def slots(dtype):
        t = torch.zeros(Cc, gy * 32, gx * 32, dtype=dtype, device="cuda")
        t[:, :H, :W] = (a.to(dtype) - b.to(dtype)).abs()
        tiles = t.view(Cc, gy, 32, gx, 32).sum(dim=(2, 4)).reshape(-1)            # block index = bx + by gx + c gx gy
        out = torch.zeros(SS_SLOTS, dtype=dtype, device="cuda")
        return out.index_add_(0, torch.arange(tiles.numel(), device="cuda") % SS_SLOTS, tiles)

    s64 = slots(torch.float64)
    sc = float(s64.max())
    _rule("ssim workspace: l1 sums per slot", err(work.view(SS_SLOTS, 2)[:, 1], s64, sc), err(slots(torch.float32), s64, sc))
    assert bool((work.view(SS_SLOTS, 2) != 0).all())             # every slot took a block's sums


@pytest.mark.parametrize("shape", SSIM_SHAPES + [(3, 577, 577)])
def test_ssim_l1_pair(shape):
    """The two-view entry points: avg_out is (f + flip(b)) / 2 bit for bit (one rounding and an exact halving); sums and maps are
    those of the single-image call on that average; both views' gradients are exactly 0.5 x the single-image gradient, b's flipped
    (with odd W the centre column maps onto itself); the gradient by the error rule against autograd of ssim_l1_pair_ref; the tie
    f = gt, b = flip(gt): an L1 sum of exactly 0 and an L1 gradient of exactly 0.
    measured on the MI355X, largest over the shapes: l1 mean 2.1e-8 / 3.5e-8, dL/df and dL/db 5.6e-7 / 5.4e-7."""
    Cc, H, W = shape
    gen = torch.Generator().manual_seed(7 * H + W)
    f, bk, gt = (torch.rand(shape, generator=gen).cuda() for _ in range(3))
    sums, maps, _, avg = _ssim_fwd(f, gt, pair_b=bk)
    want_avg = (f + bk.flip(2)) / 2
    assert torch.equal(avg, want_avg)
    sums1, maps1, _, _ = _ssim_fwd(want_avg, gt)
    assert all(torch.equal(p, q) for p, q in zip(maps, maps1))
    if shape[1] <= 100:                  # at most 1024 blocks: one add per slot, the same bits
        assert torch.equal(sums, sums1)
    up = (-0.2, 0.8)
    df, db = _ssim_bwd(f, gt, maps, up, pair_b=bk)
    d1 = _ssim_bwd(want_avg, gt, maps1, up)
    assert torch.equal(df, 0.5 * d1) and torch.equal(db, df.flip(2))
    if W % 2:
        assert torch.equal(db[:, :, W // 2], df[:, :, W // 2])
    w = ssim_window()
    outs = {}
    for dt in (torch.float64, torch.float32):
        fl, bl = f.to(dt).requires_grad_(True), bk.to(dt).requires_grad_(True)
        s, l1 = ssim_l1_pair_ref(fl, bl, gt.to(dt), w)
        outs[dt] = (s.detach(), l1.detach()) + torch.autograd.grad(up[0] * s + up[1] * l1, (fl, bl))
    s64, l64, f64, b64 = outs[torch.float64]
    s32, l32, f32_, b32 = outs[torch.float32]
    n = f.numel()
    _rule(f"pair {shape} ssim mean", abs(float(sums[0].double() / n) - float(s64)), abs(float(s32.double()) - float(s64)))
    _rule(f"pair {shape} l1 mean", abs(float(sums[1].double() / n) - float(l64)), abs(float(l32.double()) - float(l64)))
    sc = float(f64.abs().max())
    _rule(f"pair {shape} dL/df", err(df, f64, sc), err(f32_, f64, sc))
    _rule(f"pair {shape} dL/db", err(db, b64, sc), err(b32, b64, sc))
    # the tie
    sums_t, maps_t, _, avg_t = _ssim_fwd(gt, gt, pair_b=gt.flip(2).contiguous())
    assert torch.equal(avg_t, gt) and float(sums_t[1]) == 0.0
    assert abs(float(sums_t[0].double() / n) - 1.0) <= 4 * EPS32
    dft, dbt = _ssim_bwd(gt, gt, maps_t, (0.0, 1.0), pair_b=gt.flip(2).contiguous())
    assert not dft.any() and not dbt.any()


# ================================================================================================================ regularisers
def _regs_inputs(counts, seed):
    gen = torch.Generator().manual_seed(seed)
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    n = offs[-1]
    scaling = (torch.rand(n, 3, generator=gen) * 0.1 + 0.01).cuda()
    op = (torch.rand(n, 1, generator=gen) * 2 - 1).cuda()
    mask = op.view(-1) > 0
    for lo, hi in zip(offs[:-1], offs[1:]):          # a render of one or two Gaussians keeps something alive
        if hi > lo and not mask[lo:hi].any():
            op[lo] = 0.5
            mask[lo] = True
    return scaling, op, mask, offs


def _regs_call(scaling, op, mask, offs, g):
    """(out [2], grad_scaling [n, 3], grad_opacity [n]) through gsvc_regs_forward / gsvc_regs_backward."""
    lb, L, st = _lib()
    R, n = len(offs) - 1, offs[-1]
    seg = _i64(offs)
    m8 = mask.contiguous().view(torch.uint8)
    npart = int(L.gsvc_regs_partial_floats(seg, R))
    sums, out, partial = _sentinel(3 * R), _sentinel(2), _sentinel(npart)
    lb.check(L.gsvc_regs_forward(lb.ptr(scaling), lb.ptr(op), lb.ptr(m8), seg, R, lb.ptr(sums), lb.ptr(partial), lb.ptr(out), st),
             "gsvc_regs_forward")
    assert _written(sums, 3 * R) and _written(out, 2) and _written(partial, npart)
    gs, go = _sentinel(3 * n), _sentinel(n)
    gout = torch.tensor(g, dtype=torch.float32, device="cuda")
    lb.check(L.gsvc_regs_backward(lb.ptr(scaling), lb.ptr(m8), seg, R, lb.ptr(sums), lb.ptr(gout), lb.ptr(gs), lb.ptr(go), st),
             "gsvc_regs_backward")
    assert _written(gs, 3 * n) and _written(go, n)
    return out[:2], gs[:3 * n].view(n, 3), go[:n]


def _regs_ref_all(scaling, op, mask, offs, g, dtype):
    s, o = scaling.to(dtype).requires_grad_(True), op.to(dtype).requires_grad_(True)
    a, b = regs_ref(s, o, mask, offs)
    ds, do = torch.autograd.grad(g[0] * a + g[1] * b, (s, o))
    return a.detach(), b.detach(), ds, do


def _regs_check(tag, scaling, op, mask, offs, g=(3.0, 0.5)):
    out, gs, go = _regs_call(scaling, op, mask, offs, g)
    a64, b64, ds64, _ = _regs_ref_all(scaling, op, mask, offs, g, torch.float64)
    a32, b32, ds32, _ = _regs_ref_all(scaling, op, mask, offs, g, torch.float32)
    _rule(f"{tag} scaling term", err(out[0], a64, abs(float(a64))), err(a32, a64, abs(float(a64))))
    _rule(f"{tag} opacity term", err(out[1], b64, abs(float(b64))), err(b32, b64, abs(float(b64))))
    sc = float(ds64.abs().max())
    _rule(f"{tag} grad_scaling", err(gs, ds64, sc), err(ds32, ds64, sc))
    g1 = torch.tensor(g[1], dtype=torch.float32, device="cuda")
    for lo, hi in zip(offs[:-1], offs[1:]):
        if hi > lo:
            assert torch.equal(go[lo:hi], (-g1 / torch.tensor(float(hi - lo), device="cuda")).expand(hi - lo))
    return out, gs, go


def test_regs_eight_renders_and_the_second_reduction_trip():
    """R = 8 with Gaussian counts [1, 1023, 1024, 1025, 0, 263 169, 37, 4096]: 263 169 = 257 * 1024 + 1 -> 258 blocks, so
    reduce_partials takes a second trip with a partial last block.  The empty render makes both outputs NaN by design (0 / 0);
    without it: values on |ref|, grad_scaling on its maximum, grad_opacity exactly -g1 / float(count_r).  R = 1 and R = 2 likewise.
    measured on the MI355X (this and the next test): the two terms 8.3e-8 / 1.1e-7, grad_scaling 7.9e-8 / 9.6e-8."""
    counts = [1, 1023, 1024, 1025, 0, 263169, 37, 4096]
    scaling, op, mask, offs = _regs_inputs(counts, 1)
    out, gs, go = _regs_call(scaling, op, mask, offs, (3.0, 0.5))
    assert torch.isnan(out[0]) and torch.isnan(out[1])
    offs7 = [o for i, o in enumerate(offs) if i == 0 or offs[i] != offs[i - 1]]
    assert len(offs7) == 8
    out7, gs7, go7 = _regs_check("regs R=7", scaling, op, mask, offs7)
    assert torch.equal(gs, gs7) and torch.equal(go, go7)          # the gradients do not depend on the empty render
    _regs_check("regs R=1", *_regs_inputs([1025], 2))
    _regs_check("regs R=2", *_regs_inputs([37, 1024], 3))


def test_regs_dead_render_and_nine_renders():
    """A render whose mask is all false: out[0] is NaN and out[1] finite and right; that render's grad_scaling is exactly zero (not
    NaN), the other renders' gradients finite and right.  R = 9 is refused."""
    lb, L, st = _lib()
    scaling, op, mask, offs = _regs_inputs([700, 1300, 41], 4)
    mask = mask.clone()
    mask[offs[1]:offs[2]] = False
    g = (3.0, 0.5)
    out, gs, go = _regs_call(scaling, op, mask, offs, g)
    a64, b64, ds64, _ = _regs_ref_all(scaling, op, mask, offs, g, torch.float64)
    a32, b32, ds32, _ = _regs_ref_all(scaling, op, mask, offs, g, torch.float32)
    assert torch.isnan(out[0]) and torch.isnan(a64) and torch.isfinite(out[1])
    _rule("regs dead render opacity term", err(out[1], b64, abs(float(b64))), err(b32, b64, abs(float(b64))))
    assert not gs[offs[1]:offs[2]].any() and not torch.isnan(gs).any()
    live = torch.ones(offs[-1], dtype=torch.bool, device="cuda")
    live[offs[1]:offs[2]] = False
    sc = float(ds64[live].abs().max())
    assert bool(torch.isfinite(gs[live]).all()) and sc > 0
    _rule("regs dead render grad_scaling of the others", err(gs[live], ds64[live], sc), err(ds32[live], ds64[live], sc))
    g1 = torch.tensor(g[1], dtype=torch.float32, device="cuda")
    assert torch.equal(go[offs[1]:offs[2]], (-g1 / torch.tensor(1300.0, device="cuda")).expand(1300))
    # nine renders
    offs9 = list(range(0, 100, 10))
    s9, o9, m9 = scaling[:90], op[:90], mask[:90].contiguous().view(torch.uint8)
    sums, outb, partial, gs9, go9 = _sentinel(27), _sentinel(2), _sentinel(64), _sentinel(270), _sentinel(90)
    gout = torch.ones(2, device="cuda")
    assert int(L.gsvc_regs_partial_floats(_i64(offs9[:9]), 8)) == 24
    with pytest.raises(lb.GsvcError, match="regs_forward: 1..8 renders"):
        lb.check(L.gsvc_regs_forward(lb.ptr(s9), lb.ptr(o9), lb.ptr(m9), _i64(offs9), 9, lb.ptr(sums), lb.ptr(partial), lb.ptr(outb), st),
                 "gsvc_regs_forward")
    with pytest.raises(lb.GsvcError, match="regs_backward: 1..8 renders"):
        lb.check(L.gsvc_regs_backward(lb.ptr(s9), lb.ptr(m9), _i64(offs9), 9, lb.ptr(sums), lb.ptr(gout), lb.ptr(gs9), lb.ptr(go9), st),
                 "gsvc_regs_backward")
    torch.cuda.synchronize()
    assert all(_untouched(t) for t in (sums, outb, partial, gs9, go9))


# ================================================================================================================ optical flow
X_MIN, Y_MIN, SCALE = -1.0, -0.75, 32.0
FLOW_H, FLOW_W, X_PIX_MAX, Y_PIX_MAX = 48, 80, 64, 48


def _coord(p, lo):
    """The fp32 world coordinate whose pixel coordinate (v - lo) * 32 is exactly p (p a multiple of 2^-17 in [-1, 80])."""
    v = np.float32(lo) + np.float32(p) / np.float32(32.0)
    assert float(v) == lo + p / 32.0 and float((v - np.float32(lo)) * np.float32(32.0)) == p
    return v


def _below(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


# (x pixel coordinate, y pixel coordinate, accepted, pixel it lands on); None: see _constructed
_EDGE = [
    (10.5, 20.0, True, (10, 20)),          # k + 0.5, k even: rounds to even
    (11.5, 20.0, True, (12, 20)),          # k + 0.5, k odd: rounds to even
    (-0.5, 20.0, True, (0, 20)),           # rounds to -0, accepted as pixel 0
    ("below -0.5", 20.0, False, None),     # the next coordinate below: rounds to -1
    (63.5, 20.0, False, None),             # rounds to 64 = x_pix_max
    (64.0, 20.0, False, None),
    ("below 63.5", 20.0, True, (63, 20)),
    (30.0, 10.5, True, (30, 10)),
    (30.0, 11.5, True, (30, 12)),
    (30.0, -0.5, True, (30, 0)),
    (30.0, "below -0.5", False, None),
    (30.0, 47.5, False, None),             # rounds to 48 = y_pix_max
    (30.0, 48.0, False, None),
    (30.0, "below 47.5", True, (30, 47)),
    (60.0, 21.0, True, (60, 21)),          # px >= 48 with py valid: the row stride of the flow field is flow_w = 80, not 64 or 48
    (20.0, 22.0, True, (20, 22)),          # flow entry 64 = 2 * scale, partner displaced by exactly 2.0: ex == 0
]
EX0 = len(_EDGE) - 1


def _constructed():
    """World xy of the constructed Gaussians.  With x_min = -1 and y_min = -0.75 the coordinate just below the one that gives pixel
    coordinate -0.5 gives -0.5 - 2^-18 (x) and -0.5 - 2^-19 (y): the next float below -0.5 itself has no fp32 pre-image here; the
    "below" cases take the nearest coordinate whose fp32 product is below the tie (at most 2^-17 below it)."""
    xy = np.zeros((len(_EDGE), 2), dtype=np.float32)
    for i, (px, py, _, _) in enumerate(_EDGE):
        for c, (p, lo) in enumerate(((px, X_MIN), (py, Y_MIN))):
            if isinstance(p, str):
                base = float(p.split()[1])
                v = _below(_coord(base, lo))
                while float((v - np.float32(lo)) * np.float32(32.0)) >= base:      # v - lo may round back up: one more step down
                    v = _below(v)
                prod = float((v - np.float32(lo)) * np.float32(32.0))
                assert prod < base and base - prod <= 2.0 ** -17 and float(np.rint(np.float32(prod))) == np.floor(base)
            else:
                v = _coord(p, lo)
            xy[i, c] = v
    return torch.from_numpy(xy)


def _optical_render(rows, A, K, seed, forced):
    """A render of ``rows`` visible anchors out of A (the first ``forced`` anchors among them), K Gaussians each, masks ~70 %."""
    gen = torch.Generator().manual_seed(seed)
    rest = forced + torch.randperm(A - forced, generator=gen)[:rows - forced]
    vis = torch.cat([torch.arange(forced), rest.sort().values]) if rows else torch.zeros(0, dtype=torch.long)
    n = rows * K
    world = torch.stack([torch.rand(n, generator=gen) * 2.4 - 1.2, torch.rand(n, generator=gen) * 1.8 - 0.9, torch.rand(n, generator=gen)], 1)
    mask = torch.rand(n, generator=gen) < 0.7
    return vis, world, mask


def _optical_scene(rows1, K, seed, edges=True):
    """Two renders over A = rows1 / 0.6 anchors with different visible sets; the constructed Gaussians sit at slot 0 of anchors
    0 .. len(_EDGE) - 1, alive in both renders."""
    M = len(_EDGE) if edges else 0
    assert rows1 >= M
    A = max(int(rows1 / 0.6), rows1 + 1, M + 1)
    rows2 = min(A, max(M, int(0.6 * A)))
    vis1, w1, m1 = _optical_render(rows1, A, K, seed, M)
    vis2, w2, m2 = _optical_render(rows2, A, K, seed + 1, M)
    flow = 2 * torch.randn(2, FLOW_H, FLOW_W, generator=torch.Generator().manual_seed(seed + 2))
    if edges:
        idx = torch.arange(M) * K
        w1[idx, :2] = _constructed()
        m1[idx] = True
        m2[idx] = True
        flow[0, 22, 20] = 64.0
        w2[EX0 * K, 0] = w1[EX0 * K, 0] + 2.0
    return A, (vis1.cuda(), w1.cuda(), m1.cuda()), (vis2.cuda(), w2.cuda(), m2.cuda()), flow.cuda()


def _optical_single(A, r1, r2, flow, K, g):
    lb, L, st = _lib()
    (vis1, w1, m1), (vis2, w2, m2) = r1, r2
    n1, n2 = w1.shape[0], w2.shape[0]
    blocks = max((n1 + 255) // 256, 1)
    table, partner = _sentinel_i32(A * K), _sentinel_i32(n1)
    sums, partial = _sentinel(2), _sentinel(2 * blocks)
    lb.check(L.gsvc_optical_forward(lb.ptr(w1), lb.ptr(m1.view(torch.uint8)), lb.ptr(vis1), n1, lb.ptr(w2), lb.ptr(m2.view(torch.uint8)),
                                    lb.ptr(vis2), n2, K, A, lb.ptr(flow), FLOW_H, FLOW_W, X_MIN, Y_MIN, SCALE, X_PIX_MAX, Y_PIX_MAX,
                                    lb.ptr(table), lb.ptr(partner), lb.ptr(sums), lb.ptr(partial), st), "gsvc_optical_forward")
    assert _written(sums, 2) and _written(partner, n1) and _written(table, A * K)
    assert bool((partial.view(torch.int32)[2 * ((n1 + 255) // 256):] == SENTINEL).all())
    g1, g2 = _sentinel(3 * n1), _sentinel(3 * n2)
    gout = torch.tensor([g], dtype=torch.float32, device="cuda")
    lb.check(L.gsvc_optical_backward(lb.ptr(partner), n1, n2, lb.ptr(sums), lb.ptr(gout), lb.ptr(g1), lb.ptr(g2), st), "gsvc_optical_backward")
    assert _written(g1, 3 * n1) and _written(g2, 3 * n2)
    return sums[:2], g1[:3 * n1].view(n1, 3), g2[:3 * n2].view(n2, 3)


def _pair_ref(r1, r2, flow, K, dtype):
    (vis1, w1, m1), (vis2, w2, m2) = r1, r2
    return optical_pair_ref(w1.to(dtype), m1, vis1, w2.to(dtype), m2, vis2, flow, K, X_MIN, Y_MIN, SCALE, X_PIX_MAX, Y_PIX_MAX)


def _expected_grad(s, g, n):
    """+-fp32(g / (2.0f * n)) with the reference's sign pattern, column 2 zero."""
    k = torch.tensor(g, dtype=torch.float32, device="cuda") / (2.0 * torch.tensor(float(n), dtype=torch.float32, device="cuda"))
    return torch.cat([s.float() * k, torch.zeros(s.shape[0], 1, device="cuda")], 1)


OPTICAL_SIZES = [(1, 256), (1, 257), (1, 65800), (3, 86), (3, 257), (10, 26), (10, 257)]


@pytest.mark.parametrize("K,rows1", OPTICAL_SIZES)
def test_optical_single_pair(K, rows1):
    """n1 = rows1 * K Gaussians (K * ceil(256 / K), 257 K, and 65 800 for K = 1: 258 blocks, the finalize's second trip), ~60 % of the
    anchors visible per render with different visible sets, masks ~70 %, x_pix_max = 64 < flow_w = 80.  The constructed Gaussians
    (half-integer ties to even, -0.5 -> pixel 0, the bounds themselves, px >= 48, ex == 0) are accepted or rejected as the table
    says and as optical_pair_ref says; the loss on |ref| by the error rule, the count exact, the gradients exactly
    +-fp32(g / (2.0f n)) in columns 0 and 1 with the reference's signs, column 2 and every unpaired Gaussian exactly 0.
    measured on the MI355X, largest over the sizes and the batched layouts: loss 1.2e-7 / 1.8e-7."""
    A, r1, r2, flow = _optical_scene(rows1, K, 1000 * K + rows1)
    g = 0.7
    sums, g1, g2 = _optical_single(A, r1, r2, flow, K, g)
    l64, n, (s1, s2) = _pair_ref(r1, r2, flow, K, torch.float64)
    l32, n32, _ = _pair_ref(r1, r2, flow, K, torch.float32)
    assert n == n32 and n >= 8 and float(sums[1]) == float(n)
    _rule(f"optical K={K} rows={rows1} loss", err(sums[0].double() / (2 * n), l64, abs(float(l64))), err(l32, l64, abs(float(l64))))
    # the constructed rows, one by one: the reference agrees with the table, the kernel with the reference
    idx = torch.arange(len(_EDGE), device="cuda") * K
    accepted = torch.tensor([e[2] for e in _EDGE], device="cuda")
    assert torch.equal(s1[idx].abs().sum(1) > 0, accepted)
    assert float(s1[EX0 * K, 0]) == 0.0 and float(s1[EX0 * K, 1]) != 0.0
    want1, want2 = _expected_grad(s1, g, n), _expected_grad(s2, g, n)
    assert torch.equal(g1, want1) and torch.equal(g2, want2)
    assert torch.equal(g1[idx].abs().sum(1) > 0, accepted) and float(g1[EX0 * K, 0]) == 0.0
    assert int((want1[:, 0] != 0).sum()) >= n - 4 and not g1[:, 2].any() and not g2[:, 2].any()
    # the accepted ones land on the pixel of the table: moving that pixel's flow moves the loss by exactly that pair's share
    (vis1, w1, m1), (vis2, w2, m2) = r1, r2
    for i, (_, _, ok, pix) in enumerate(_EDGE):
        if ok and i != EX0:
            flow2 = flow.clone()
            flow2[1, pix[1], pix[0]] += 4096.0
            la, _, _ = _pair_ref(r1, r2, flow2, K, torch.float64)
            assert abs(float(la) - float(l64)) > 1.0 / n, (i, pix)
    flow2 = flow.clone()
    for _, _, ok, pix in _EDGE:
        if ok:
            flow2[1, pix[1], pix[0]] += 4096.0
    sums_b, _, _ = _optical_single(A, r1, r2, flow2, K, g)
    lb64, nb, _ = _pair_ref(r1, r2, flow2, K, torch.float64)
    lb32, _, _ = _pair_ref(r1, r2, flow2, K, torch.float32)
    assert nb == n and float(sums_b[1]) == float(n)
    _rule(f"optical K={K} rows={rows1} loss, flow moved under the constructed pixels",
          err(sums_b[0].double() / (2 * n), lb64, abs(float(lb64))), err(lb32, lb64, abs(float(lb64))))


def test_optical_single_pair_empty_renders():
    """n1 = 0 and n2 = 0 return sums (0, 0); the other render's gradient is zeros."""
    K = 3
    A, r1, r2, flow = _optical_scene(40, K, 5, edges=False)
    empty = (r1[0][:0].contiguous(), r1[1][:0].contiguous(), r1[2][:0].contiguous())
    sums, g1, g2 = _optical_single(A, empty, r2, flow, K, 1.0)
    assert float(sums[0]) == 0.0 and float(sums[1]) == 0.0 and g1.numel() == 0 and not g2.any()
    sums, g1, g2 = _optical_single(A, r1, empty, flow, K, 1.0)
    assert float(sums[0]) == 0.0 and float(sums[1]) == 0.0 and g2.numel() == 0 and not g1.any()


OPTICAL_LAYOUTS = {
    "f1 b1 f2 b2": ((720, 700, 730, 710), ((0, 2), (1, 3))),
    "sources last": ((720, 700, 730, 710), ((2, 0), (3, 1))),
    "a render in no pair": ((720, 300, 730), ((0, 2),)),
    "one short source": ((720, 40, 730, 710), ((0, 2), (1, 3))),
}


def _optical_many_buffers(renders, pairs, K, A):
    goff = [0]
    for _, w, _ in renders:
        goff.append(goff[-1] + w.shape[0])
    world = torch.cat([w for _, w, _ in renders]).contiguous()
    mask = torch.cat([m for _, _, m in renders]).contiguous()
    vis = torch.cat([v for v, _, _ in renders]).contiguous()
    return goff, world, mask, vis


@pytest.mark.parametrize("layout", list(OPTICAL_LAYOUTS))
def test_optical_many(layout):
    """The batched entry points over renders that are row ranges of one set of tensors: the loss against the sum of optical_pair_ref
    over the pairs, the gradient exact per pair as in the single-pair test and EVERY element written (the autograd wrapper
    allocates it with torch.empty): zeros for a render that is in no pair, for the blocks that lie wholly past a short source
    render, for unpaired Gaussians and in column 2."""
    lb, L, st = _lib()
    rows, pairs = OPTICAL_LAYOUTS[layout]
    K, A = 3, 1200
    renders = []
    for r, nrows in enumerate(rows):
        v, w, m = _optical_render(nrows, A, K, 50 + r, 0)
        renders.append((v.cuda(), w.cuda(), m.cuda()))
    flow = (2 * torch.randn(2, FLOW_H, FLOW_W, generator=torch.Generator().manual_seed(9))).cuda()
    goff, world, mask, vis = _optical_many_buffers(renders, pairs, K, A)
    R, P, total = len(rows), len(pairs), goff[-1]
    off, src, dst = _i64(goff), _i32([p[0] for p in pairs]), _i32([p[1] for p in pairs])
    npart = int(L.gsvc_optical_many_partial_floats(off, R, src, dst, P, K))
    assert npart == 2 * P * ((max(renders[p[0]][1].shape[0] for p in pairs) + 255) // 256)
    table, partner = _sentinel_i32(R * A), _sentinel_i32(total)
    sums, partial, loss = _sentinel(2 * P), _sentinel(npart), _sentinel(1)
    lb.check(L.gsvc_optical_many_forward(lb.ptr(world), lb.ptr(mask.view(torch.uint8)), lb.ptr(vis), off, R, src, dst, P, K, A, lb.ptr(flow),
                                         FLOW_H, FLOW_W, X_MIN, Y_MIN, SCALE, X_PIX_MAX, Y_PIX_MAX, lb.ptr(table), lb.ptr(partner),
                                         lb.ptr(sums), lb.ptr(partial), lb.ptr(loss), st), "gsvc_optical_many_forward")
    assert _written(table, R * A) and _written(sums, 2 * P) and _written(partial, npart) and _written(loss, 1)
    assert bool((partner[total:] == SENTINEL).all())
    g = 0.7
    gw = _sentinel(3 * total)
    gout = torch.tensor([g], dtype=torch.float32, device="cuda")
    lb.check(L.gsvc_optical_many_backward(lb.ptr(partner), lb.ptr(vis), off, R, src, dst, P, K, A, lb.ptr(table), lb.ptr(sums), lb.ptr(gout),
                                          lb.ptr(gw), st), "gsvc_optical_many_backward")
    assert _written(gw, 3 * total)
    gw = gw[:3 * total].view(total, 3)
    want = torch.zeros(total, 3, device="cuda")
    l64 = l32 = 0.0
    for p, (a, b) in enumerate(pairs):
        la, n, (s1, s2) = _pair_ref(renders[a], renders[b], flow, K, torch.float64)
        lc, n32, _ = _pair_ref(renders[a], renders[b], flow, K, torch.float32)
        assert n == n32 and n > 5 and float(sums[2 * p + 1]) == float(n)
        l64, l32 = l64 + float(la), l32 + float(lc.double())
        want[goff[a]:goff[a + 1]] = _expected_grad(s1, g, n)
        want[goff[b]:goff[b + 1]] = _expected_grad(s2, g, n)
    _rule(f"optical many '{layout}' loss", abs(float(loss[0]) - l64) / abs(l64), abs(l32 - l64) / abs(l64))
    assert torch.equal(gw, want)
    in_pair = {r for p in pairs for r in p}
    for r in range(R):
        if r not in in_pair:
            assert goff[r + 1] > goff[r] and not gw[goff[r]:goff[r + 1]].any()


def test_optical_many_refusals():
    lb, L, st = _lib()
    K, A = 3, 100
    goff = _i64([0, 30, 60, 90, 120])
    world, mask, vis = torch.rand(120, 3, device="cuda"), torch.ones(120, dtype=torch.uint8, device="cuda"), torch.arange(40, device="cuda") % 10
    flow = torch.zeros(2, FLOW_H, FLOW_W, device="cuda")
    table, partner, sums, partial, loss, gw = _sentinel_i32(4 * A), _sentinel_i32(120), _sentinel(4), _sentinel(8), _sentinel(1), _sentinel(360)
    gout = torch.ones(1, device="cuda")
    for pairs in (((0, 2), (0, 3)), ((0, 2), (3, 2)), ((1, 1),)):
        P = len(pairs)
        src, dst = _i32([p[0] for p in pairs]), _i32([p[1] for p in pairs])
        assert int(L.gsvc_optical_many_partial_floats(goff, 4, src, dst, P, K)) == -1
        with pytest.raises(lb.GsvcError, match="optical_many_forward: 2..8 renders of whole rows, 1..4 disjoint pairs"):
            lb.check(L.gsvc_optical_many_forward(lb.ptr(world), lb.ptr(mask), lb.ptr(vis), goff, 4, src, dst, P, K, A, lb.ptr(flow), FLOW_H,
                                                 FLOW_W, X_MIN, Y_MIN, SCALE, X_PIX_MAX, Y_PIX_MAX, lb.ptr(table), lb.ptr(partner),
                                                 lb.ptr(sums), lb.ptr(partial), lb.ptr(loss), st), "gsvc_optical_many_forward")
        with pytest.raises(lb.GsvcError, match="optical_many_backward: bad arguments"):
            lb.check(L.gsvc_optical_many_backward(lb.ptr(partner), lb.ptr(vis), goff, 4, src, dst, P, K, A, lb.ptr(table), lb.ptr(sums),
                                                  lb.ptr(gout), lb.ptr(gw), st), "gsvc_optical_many_backward")
    torch.cuda.synchronize()
    assert all(_untouched(t) for t in (table, partner, sums, partial, loss, gw))


# ================================================================================================================ rate
RATE_SHAPES = [(1, 1), (3, 64), (2, 65), (5, 130), (20000, 50)]
_rate_cache = {}


def _rate_inputs(n, c):
    """numpy.default_rng(5): x = 2 N(0, 1), mean = N(0, 1), scale = U(0.05, 2), Q = U(0.05, 1) per row (drawn once per shape)."""
    if (n, c) not in _rate_cache:
        rng = np.random.default_rng(5)
        x = (2 * rng.standard_normal((n, c))).astype(np.float32)
        mean = rng.standard_normal((n, c)).astype(np.float32)
        scale = rng.uniform(0.05, 2, (n, c)).astype(np.float32)
        Q = rng.uniform(0.05, 1, n).astype(np.float32)
        w = rng.uniform(0.0, 1.0, (n, c)).astype(np.float32)
        _rate_cache[(n, c)] = tuple(torch.from_numpy(a).cuda() for a in (x, mean, scale, Q, w))
    return _rate_cache[(n, c)]


def _rate_bounds(mode, x, Q, q_scalar):
    """(x_lo, x_hi, bounds_per_row) as device tensors."""
    n = x.shape[0]
    if mode == "scalar":
        qm = Q.mean() if q_scalar is None else torch.tensor(q_scalar, device="cuda")
        return (x.mean() - 15000.0 * qm).reshape(1), (x.mean() + 15000.0 * qm).reshape(1), 0
    if mode == "inf":
        return torch.full((n,), -float("inf"), device="cuda"), torch.full((n,), float("inf"), device="cuda"), 1
    lo, hi = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")       # three "renders", a few per cent of x clamped in each
    cuts = [0, n // 3, (2 * n) // 3, n]
    for (a, b), (l, h) in zip(zip(cuts[:-1], cuts[1:]), ((-4.2, 4.5), (-3.5, 5.0), (-5.0, 3.8))):
        lo[a:b], hi[a:b] = l, h
    return lo, hi, 1


def _rate_ref(x, mean, scale, qe, lo, hi, w, gs, dtype):
    """bits, unfloored likelihood, dx, dmean, dscale, the per-element terms of dQ, dweight of L = gs * sum(w * bits)."""
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (x, mean, scale, qe)]
    lo_, hi_ = (t.to(dtype) if t.numel() > 1 else float(t) for t in (lo, hi))
    bits, raw = rate_bits_ref(*leaves, lo_, hi_)
    wt = torch.ones_like(bits) if w is None else w.to(dtype)
    grads = torch.autograd.grad((bits * wt).sum() * gs, leaves)
    return (bits.detach(), raw.detach()) + grads + (bits.detach() * gs,)


def _rate_forward(x, mean, scale, Q, q_scalar, w, lo, hi, per_row, want_bits=True, preset=None):
    lb, L, st = _lib()
    n, c = x.shape
    bits = _sentinel(n * c) if want_bits else None
    bsum = scratch = None
    if preset is not None:
        bsum, scratch = _sentinel(1), _sentinel(int(L.gsvc_rate_forward_scratch_floats()))
        bsum[0] = preset
    lb.check(L.gsvc_rate_forward(lb.ptr(x), lb.ptr(mean), lb.ptr(scale), lb.ptr(Q), 0.0 if q_scalar is None else q_scalar, lb.ptr(w),
                                 lb.ptr(lo), lb.ptr(hi), per_row, n, c, lb.ptr(bits), lb.ptr(bsum), lb.ptr(scratch), st), "gsvc_rate_forward")
    assert bits is None or _written(bits, n * c)
    assert bsum is None or (_written(bsum, 1) and _untouched(scratch[min(2 * ((n * c + 255) // 256), int(L.gsvc_rate_forward_scratch_floats())):]))
    return (bits[:n * c].view(n, c) if want_bits else None), (bsum[:1] if bsum is not None else None)


RATE_OUT = ("dx", "dmean", "dscale", "dQ", "dweight")


def _rate_backward(x, mean, scale, Q, q_scalar, w, lo, hi, per_row, gs, skip=None, dq_preset=None):
    """The five outputs (None for the one named by ``skip``), each in a guarded buffer; dQ starts from zeros or ``dq_preset``."""
    lb, L, st = _lib()
    n, c = x.shape
    bufs = {k: (_zeros_guarded(n) if k == "dQ" else _sentinel(n * c)) for k in RATE_OUT}
    if dq_preset is not None:
        bufs["dQ"][:n] = dq_preset
    if skip:
        bufs[skip] = None
    gdev = None if gs is None else torch.tensor([gs], dtype=torch.float32, device="cuda")
    lb.check(L.gsvc_rate_backward(lb.ptr(x), lb.ptr(mean), lb.ptr(scale), lb.ptr(Q), 0.0 if q_scalar is None else q_scalar, lb.ptr(w),
                                  lb.ptr(lo), lb.ptr(hi), per_row, n, c, lb.ptr(gdev), *(lb.ptr(bufs[k]) for k in RATE_OUT), st),
             "gsvc_rate_backward")
    out = {}
    for k in RATE_OUT:
        m = n if k == "dQ" else n * c
        if bufs[k] is None:
            out[k] = None
            continue
        assert _written(bufs[k], m), k
        out[k] = bufs[k][:m] if k == "dQ" else bufs[k][:m].view(n, c)
    return out


def _rate_case(tag, n, c, q_mode, b_mode, weighted, gs, edges=False):
    """One forward and one backward call against the float64 reference, by the derived per-element scales."""
    x, mean, scale, Q, w = _rate_inputs(n, c)
    x = x.clone()
    q_scalar = None if q_mode == "rows" else 0.3
    Qk = Q if q_mode == "rows" else None
    lo, hi, per_row = _rate_bounds(b_mode, x, Q, q_scalar)
    edge_rows = None
    if edges:                                   # x exactly on either bound, and one ulp outside
        assert per_row and b_mode == "rows" and c >= 4
        edge_rows = torch.arange(0, n, max(n // 64, 1), device="cuda")
        x[edge_rows, 0], x[edge_rows, 1] = lo[edge_rows], hi[edge_rows]
        x[edge_rows, 2] = torch.nextafter(lo[edge_rows], torch.full_like(lo[edge_rows], -float("inf")))
        x[edge_rows, 3] = torch.nextafter(hi[edge_rows], torch.full_like(hi[edge_rows], float("inf")))
    wk = w if weighted else None
    gsv = 1.0 if gs is None else gs
    qe = (Q.reshape(-1, 1) if q_mode == "rows" else torch.full((n, 1), q_scalar, device="cuda")).expand(n, c)
    r64 = _rate_ref(x, mean, scale, qe, lo, hi, wk, gsv, torch.float64)
    r32 = _rate_ref(x, mean, scale, qe, lo, hi, wk, gsv, torch.float32)
    bits64, raw64 = r64[0], r64[1]
    lik = raw64.clamp_min(LOW_BOUND)
    ambiguous = (raw64 - LOW_BOUND).abs() <= 8 * EPS32
    left_out = int(ambiguous.sum())
    assert left_out <= int(np.ceil(5e-3 * n * c)), (left_out, n * c)     # the cap, in whole elements (one of the 192 of (3, 64) is allowed)
    keep = ~ambiguous
    bits, bsum = _rate_forward(x, mean, scale, Qk, q_scalar, wk, lo, hi, per_row, preset=3.0)
    out = _rate_backward(x, mean, scale, Qk, q_scalar, wk, lo, hi, per_row, gs)
    assert bool(torch.isfinite(bits).all()) and float(bits.max()) <= 16.0 and all(bool(torch.isfinite(v).all()) for v in out.values())
    amp = 1 + 1 / lik

    def each(got, ref, sc):
        q = err_each(got, ref, sc)[keep]
        return float(q.max()) if q.numel() else 0.0

    sc_bits = EPS32 * (1 / (lik * np.log(2.0)) + bits64.abs())
    _rule(f"{tag} bits", each(bits, bits64, sc_bits), each(r32[0], bits64, sc_bits))
    for k, i in (("dx", 2), ("dmean", 3), ("dscale", 4)):
        sc = r64[i].abs() * amp
        _rule(f"{tag} {k}", each(out[k], r64[i], sc), each(r32[i], r64[i], sc))
    sc_w = sc_bits * abs(gsv)
    _rule(f"{tag} dweight", each(out["dweight"], r64[6], sc_w), each(r32[6], r64[6], sc_w))
    rows_ok = ~ambiguous.any(1)
    sc_q = (r64[5].abs() * amp).sum(1)
    eq = lambda got: float(err_each(got, r64[5].sum(1), sc_q)[rows_ok].max()) if bool(rows_ok.any()) else 0.0  # noqa: E731
    _rule(f"{tag} dQ", eq(out["dQ"]), eq(r32[5].sum(1)))
    wt64 = torch.ones_like(bits64) if wk is None else wk.double()
    sc_s = float((wt64 * bits64).abs().sum())
    s64 = 3.0 + float((wt64 * bits64).sum())
    s32 = float((torch.tensor(3.0, device="cuda") + ((r32[0] * wk).sum() if wk is not None else r32[0].sum())).double())
    sum_err = (f"{tag} bits_sum (added to 3.0)", abs(float(bsum[0].double()) - s64) / sc_s, abs(s32 - s64) / sc_s)      # test_rate_bits_sum
    if edges:
        passes, sure = r64[2][edge_rows, :2] != 0, keep[edge_rows, :2]
        assert bool(passes.any()) and torch.equal((out["dx"][edge_rows, :2] != 0) & sure, passes & sure)
        assert not out["dx"][edge_rows, 2:4].any() and not r64[2][edge_rows, 2:4].any()
        live, sure = r64[3][edge_rows, 2:4] != 0, keep[edge_rows, 2:4]
        assert bool(live.any()) and torch.equal((out["dmean"][edge_rows, 2:4] != 0) & sure, live & sure)
    return dict(x=x, mean=mean, scale=scale, Q=Qk, q_scalar=q_scalar, w=wk, lo=lo, hi=hi, per_row=per_row, gs=gs, bits=bits, out=out,
                bits64=bits64, bits32=r32[0], keep=keep, sc_s=sc_s, wt64=wt64, sum_err=sum_err)


@pytest.mark.parametrize("n,c", RATE_SHAPES)
def test_rate_shapes(n, c):
    """Per-row Q, one scalar pair of bounds from mean(x) -+ 15000 mean(Q), weights, gscale 0.37, at every shape: (1, 1), the 64-column
    loop's one, two and three trips, and (20 000, 50): 1 000 000 elements = the second, partial trip of the forward's grid-stride
    loop and the second trip of the backward's row loop.
    measured on the MI355X, largest over all rate cases at (20 000, 50) [at the smaller shapes], kernel / fp32 statement: bits 4.11 /
    4.11 [2.16 / 2.16] in units of its one-ulp scale, dweight 4.26 / 4.11, dx and dmean 1.3e-3 / 8.1e-3 [8.2e-6 / 2.1e-5] (the
    fp32 statement loses more where the two densities cancel), dscale 1.2e-2 / 1.2e-2 [4.1e-6 / 3.4e-6], dQ 8.2e-8 / 8.2e-8; 1.4e-3
    of the elements within 8 eps32 of the floor and left out."""
    _rate_case(f"rate ({n}, {c}) rows/scalar", n, c, "rows", "scalar", True, 0.37)


@pytest.mark.parametrize("n,c", [(5, 130), (20000, 50)])
@pytest.mark.parametrize("q_mode", ["rows", "scalar"])
@pytest.mark.parametrize("b_mode", ["rows", "inf"])
def test_rate_modes(n, c, q_mode, b_mode):
    """Q per row and scalar x per-row bounds (three "renders", a few per cent of x clamped; x exactly on a bound: dx passes, one ulp
    outside: dx == 0 and dmean != 0) and +-inf per row; unweighted, no gscale."""
    _rate_case(f"rate ({n}, {c}) {q_mode}/{b_mode}", n, c, q_mode, b_mode, False, None, edges=(b_mode == "rows"))


def test_rate_scalar_q_scalar_bounds():
    _rate_case("rate (5, 130) scalar/scalar", 5, 130, "scalar", "scalar", True, None)
    _rate_case("rate (20000, 50) scalar/scalar", 20000, 50, "scalar", "scalar", False, 2.0)


RATE_MODES = [("rows", "scalar", True, 0.37), ("rows", "rows", False, None), ("scalar", "rows", False, None), ("rows", "inf", False, None),
              ("scalar", "inf", False, None), ("scalar", "scalar", True, None)]


@pytest.mark.parametrize("n,c", RATE_SHAPES)
def test_rate_bits_sum(n, c):
    """bits_sum = preset + sum(w * bits) on the scale sum |w * bits|, by the error rule, in every mode of the tests above (and with
    bits == NULL); the scratch past the workgroups' partials stays untouched, and bits_sum without scratch is refused.
    This test found k_rate_fwd adding its 2048 workgroup sums onto bits_sum with one float atomicAdd each: a serial fp32
    accumulation whose length and order changed from run to run, 1.8e-7 .. 1.4e-6 at (20 000, 50) against 1.1e-8 .. 1.3e-7 for the
    fp32 tensor statement (pairwise sum).  The kernel now leaves one double partial per workgroup (as a float pair) in a scratch
    argument and a one-workgroup second stage adds them in fixed order and rounds once.
    measured on the MI355X, kernel / fp32 statement, in units of sum |w * bits|: at (20 000, 50) 1.1e-8 .. 1.4e-7 for both, equal to
    the digit in all seven cases; at the four small shapes 2.7e-8 .. 3.3e-6 / 4.6e-8 .. 3.1e-6."""
    modes = RATE_MODES if c >= 4 else RATE_MODES[:1]
    errs = []
    for q_mode, b_mode, weighted, gs in modes:
        r = _rate_case(f"rate ({n}, {c}) {q_mode}/{b_mode}", n, c, q_mode, b_mode, weighted, gs)
        errs.append(r["sum_err"])
        if weighted:
            _, only = _rate_forward(r["x"], r["mean"], r["scale"], r["Q"], r["q_scalar"], r["w"], r["lo"], r["hi"], r["per_row"],
                                    want_bits=False, preset=-7.5)
            s64 = -7.5 + float((r["wt64"] * r["bits64"]).sum())
            s32 = float((torch.tensor(-7.5, device="cuda") + (r["bits32"] * r["w"]).sum()).double())
            errs.append((f"rate ({n}, {c}) {q_mode}/{b_mode} bits_sum alone", abs(float(only[0].double()) - s64) / r["sc_s"],
                         abs(s32 - s64) / r["sc_s"]))
    for tag, e_k, e32 in errs:
        if PRINT:
            print(f"LOSS_ERR {tag}: kernel {e_k:.3e} fp32 statement {e32:.3e}")
    for tag, e_k, e32 in errs:
        assert e_k <= 4 * e32 + 4 * EPS32, (tag, e_k, e32)
    lb, L, st = _lib()
    x, mean, scale, Q, _ = _rate_inputs(n, c)
    bsum = _sentinel(1)
    with pytest.raises(lb.GsvcError, match="rate_forward: bits_sum needs scratch"):
        lb.check(L.gsvc_rate_forward(lb.ptr(x), lb.ptr(mean), lb.ptr(scale), lb.ptr(Q), 0.0, None, None, None, 0, n, c, None, lb.ptr(bsum),
                                     None, st), "gsvc_rate_forward")
    torch.cuda.synchronize()
    assert _untouched(bsum)


@pytest.mark.parametrize("n,c", [(5, 130), (20000, 50)])
def test_rate_contracts(n, c):
    """What the callers rely on: bits do not depend on the weights; bits_sum with bits == NULL; gscale multiplies every gradient and
    nothing else; dQ is ADDED to what the buffer held (entropy_models._GaussianBits.backward zero-fills it); each of the five
    output pointers NULL in turn leaves the others bit-identical; n = 0 or c = 0 returns OK and writes nothing."""
    lb, L, st = _lib()
    r = _rate_case(f"rate ({n}, {c}) contracts", n, c, "rows", "rows", True, 0.37)
    a = (r["x"], r["mean"], r["scale"], r["Q"], r["q_scalar"])
    b = (r["lo"], r["hi"], r["per_row"])
    bits_now, _ = _rate_forward(*a, None, *b)
    assert torch.equal(bits_now, r["bits"])
    _, only_sum = _rate_forward(*a, r["w"], *b, want_bits=False, preset=-7.5)
    s64 = -7.5 + float((r["wt64"] * r["bits64"]).sum())
    assert bool(torch.isfinite(only_sum).all()) and abs(float(only_sum[0].double()) - s64) <= 1e-5 * r["sc_s"]       # the sum's accuracy: test_rate_bits_sum
    # gscale: 2.0 is an exact factor, so every gradient doubles bit for bit
    g1 = _rate_backward(*a, r["w"], *b, None)
    g2 = _rate_backward(*a, r["w"], *b, 2.0)
    assert all(torch.equal(g2[k], 2.0 * g1[k]) for k in RATE_OUT)
    # dQ accumulates
    preset = torch.randn(n, generator=torch.Generator().manual_seed(n)).cuda()
    gp = _rate_backward(*a, r["w"], *b, 0.37, dq_preset=preset)
    assert torch.equal(gp["dQ"], preset + r["out"]["dQ"]) and bool(r["out"]["dQ"].any())
    assert all(torch.equal(gp[k], r["out"][k]) for k in RATE_OUT if k != "dQ")
    # every output optional
    for skip in RATE_OUT:
        go = _rate_backward(*a, r["w"], *b, 0.37, skip=skip)
        assert all(torch.equal(go[k], r["out"][k]) for k in RATE_OUT if k != skip), skip
    # nothing to do
    bufs = [_sentinel(16) for _ in range(8)]
    for nn, cc in ((0, 4), (4, 0)):
        assert L.gsvc_rate_forward(lb.ptr(r["x"]), lb.ptr(r["mean"]), lb.ptr(r["scale"]), lb.ptr(r["Q"]), 0.0, None, None, None, 0, nn, cc,
                                   lb.ptr(bufs[0]), lb.ptr(bufs[1]), lb.ptr(bufs[7]), st) == 0
        assert L.gsvc_rate_backward(lb.ptr(r["x"]), lb.ptr(r["mean"]), lb.ptr(r["scale"]), lb.ptr(r["Q"]), 0.0, None, None, None, 0, nn, cc,
                                    None, *(lb.ptr(t) for t in bufs[2:]), st) == 0
    torch.cuda.synchronize()
    assert all(_untouched(t) for t in bufs)


# ================================================================================================================ noise quantiser
def _quant_inputs(rows_per_render, Cq, seed):
    """x = 3 randn, Q = U(0.05, 0.25), noise = U(-1/2, 1/2); in every render of at least 63 rows three whole rows at
    +(17 500, 18 500, 19 500) Q and one at -17 000 Q (a render of one row cannot be clamped: it is its own centre).  More rows above
    than below on purpose: with as much below as above the render's mean is what cancellation leaves of +-3500, and a centre
    "on |ref|" then measures the summation order, not the kernel."""
    gen = torch.Generator().manual_seed(seed)
    offs = [0]
    for r in rows_per_render:
        offs.append(offs[-1] + r)
    rows = offs[-1]
    x = 3 * torch.randn(rows, Cq, generator=gen)
    Q = 0.05 + 0.2 * torch.rand(rows, generator=gen)
    noise = torch.rand(rows, Cq, generator=gen) - 0.5
    g = torch.randn(rows, Cq, generator=gen)
    return x, Q, noise, g, offs


def _quant_outliers(x, Qrow, offs):
    for lo, hi in zip(offs[:-1], offs[1:]):
        if hi - lo >= 63:
            for j, m in enumerate((17500.0, 18500.0, 19500.0, -17000.0)):
                row = lo + 7 + 11 * j
                x[row] = m * Qrow[row]
    return x


def _quant_call(x, Qk, q_scalar, noise, g, offs, want_dq=True):
    lb, L, st = _lib()
    rows, Cq = x.shape
    R = len(offs) - 1
    off = _i64(offs)
    nscratch = int(L.gsvc_noise_quant_scratch_floats(off, R))
    scratch, centre, y = _sentinel(nscratch), _sentinel(R), _sentinel(rows * Cq)
    qs = 0.0 if q_scalar is None else q_scalar
    lb.check(L.gsvc_noise_quant_forward(lb.ptr(x), lb.ptr(Qk), qs, lb.ptr(noise), off, R, Cq, lb.ptr(scratch), lb.ptr(centre), lb.ptr(y), st),
             "gsvc_noise_quant_forward")
    assert _written(scratch, nscratch) and _written(centre, R) and _written(y, rows * Cq)
    dx, dq = _sentinel(rows * Cq), _sentinel(rows)
    lb.check(L.gsvc_noise_quant_backward(lb.ptr(g), lb.ptr(x), lb.ptr(Qk), qs, lb.ptr(noise), lb.ptr(centre), off, R, Cq, lb.ptr(dx),
                                         lb.ptr(dq) if want_dq else None, st), "gsvc_noise_quant_backward")
    assert _written(dx, rows * Cq) and (_written(dq, rows) if want_dq else _untouched(dq))
    return y[:rows * Cq].view(rows, Cq), centre[:R], dx[:rows * Cq].view(rows, Cq), dq[:rows]


def _quant_check(tag, rows_per_render, Cq, per_row, seed):
    x, Q, noise, g, offs = _quant_inputs(rows_per_render, Cq, seed)
    q_scalar = None if per_row else 0.2
    Qrow = Q if per_row else torch.full_like(Q, q_scalar)
    x = _quant_outliers(x, Qrow, offs)
    x, Q, noise, g = (t.cuda().contiguous() for t in (x, Q, noise, g))
    Qk = Q if per_row else None
    qa = Q if per_row else q_scalar
    y, centre, dx, dq = _quant_call(x, Qk, q_scalar, noise, g, offs)
    qa64 = Q.double() if per_row else q_scalar
    y64, c64, in64 = noise_quant_ref(x.double(), qa64, noise.double(), offs)
    y32, c32, in32 = noise_quant_ref(x, qa, noise, offs)
    # the clamp decision must not hang on the rounding of the centre
    live = torch.tensor([hi > lo for lo, hi in zip(offs[:-1], offs[1:])], device="cuda")
    rr = torch.repeat_interleave(torch.arange(len(offs) - 1, device="cuda"), torch.tensor(rows_per_render, device="cuda"))
    Qb = Q.double().reshape(-1, 1) if per_row else q_scalar
    dist = (x.double() / Qb - c64[rr].reshape(-1, 1)).abs()
    assert not bool(((dist >= 14000) & (dist <= 16000)).any())
    assert torch.equal(in64, in32) and torch.equal(in64, dist <= 15000)
    if any(r >= 63 for r in rows_per_render):
        assert int((~in64).sum()) == 4 * Cq * sum(r >= 63 for r in rows_per_render)
    sc = c64[live].abs()
    _rule(f"{tag} centre", err(centre[live], c64[live], sc), err(c32[live], c64[live], sc))
    Qf = Q.double().reshape(-1, 1).expand_as(y64) if per_row else torch.full_like(y64, q_scalar)
    sc_y = torch.where(in64, x.double().abs() + (noise.double() * Qf).abs(), (c64[rr].reshape(-1, 1).abs() + 15000.0) * Qf)
    _rule(f"{tag} y", err(y, y64, sc_y), err(y32, y64, sc_y))
    assert torch.equal(dx, torch.where(in64, g, torch.zeros_like(g)))
    _, dq64, sq64 = noise_quant_grads(g.double(), x.double(), qa64, noise.double(), offs)
    _, dq32, _ = noise_quant_grads(g, x, qa, noise, offs)
    _rule(f"{tag} dq", err(dq, dq64, sq64), err(dq32, dq64, sq64))
    return (x, Qk, q_scalar, noise, g, offs), (y, centre, dx, dq), live


@pytest.mark.parametrize("per_row", [True, False])
def test_noise_quant_eight_renders(per_row):
    """R = 8, rows per render [0, 1, 63, 64, 65, 16 449, 300, 1111], C = 3: 16 449 rows = 257 slabs of 64 + 1, so k_quant_centre takes
    its second trip.  The empty render changes no other render's outputs: bit-identical to the call that leaves it out.
    measured on the MI355X, largest over all quantiser cases: centre 1.9e-7 / 7.2e-8 of |centre|."""
    rows = [0, 1, 63, 64, 65, 16449, 300, 1111]
    (x, Qk, q_scalar, noise, g, offs), (y, centre, dx, dq), live = _quant_check(f"quant R=8 per_row={per_row}", rows, 3, per_row, 21)
    y7, c7, dx7, dq7 = _quant_call(x, Qk, q_scalar, noise, g, offs[1:])
    assert torch.equal(y, y7) and torch.equal(centre[1:], c7) and torch.equal(dx, dx7) and torch.equal(dq, dq7)
    if not per_row:                 # scalar Q and no gradient for it: nothing but dx is written
        _quant_call(x, None, q_scalar, noise, g, offs, want_dq=False)


@pytest.mark.parametrize("per_row", [True, False])
@pytest.mark.parametrize("Cq", [1, 30, 50, 64, 100, 256])
def test_noise_quant_row_lengths(Cq, per_row):
    """R = 3, rows [300, 0, 700] for C in {1, 30, 50, 64, 100, 256}: the backward takes rpb = 256 / C = 256, 8, 5, 4, 2, 1 rows per
    block; 50 and 100 leave idle lanes, 256 is one row per block.
    measured on the MI355X, largest over this and the test above: y 1.7e-7 / 1.7e-7, dq 2.3e-7 / 1.3e-7."""
    _quant_check(f"quant C={Cq} per_row={per_row}", [300, 0, 700], Cq, per_row, 100 + Cq)


def test_noise_quant_backward_refuses_257_columns():
    lb, L, st = _lib()
    x = torch.randn(4, 257, device="cuda")
    dx, dq, centre = _sentinel(4 * 257), _sentinel(4), torch.zeros(1, device="cuda")
    with pytest.raises(lb.GsvcError, match="noise_quant_backward: 1..8 renders, 0 < C <= 256"):
        lb.check(L.gsvc_noise_quant_backward(lb.ptr(x), lb.ptr(x), None, 0.2, lb.ptr(x), lb.ptr(centre), _i64([0, 4]), 1, 257, lb.ptr(dx),
                                             lb.ptr(dq), st), "gsvc_noise_quant_backward")
    torch.cuda.synchronize()
    assert _untouched(dx) and _untouched(dq)
