"""The 13 entry points of csrc/generate.hip that were reached only through their autograd wrappers or the step plan (gsvc_embed_pe,
gsvc_gather_rows_forward / _backward / _backward_ranked, gsvc_plan_masks, gsvc_plan_scans, gsvc_compact_by_scan,
gsvc_ctx_post_forward / _backward, gsvc_q_rows_forward / _backward, gsvc_segment_rows_sum, gsvc_film_row_maps) called through
gsvc_amd._lib on guarded raw buffers, each against the float64 run of its plain tensor statement in tests/_gen_kernel_refs.py.

Error rule: e_kernel <= 4 * e32 + 4 * eps32 for outputs that involve expf, sincosf, a sigmoid or a reordered sum, both errors
against the float64 statement on the scale the case names, e32 being the error of the same statement run in fp32 on the GPU on the
same inputs (never the kernel's own output).  Everything else is exact: copies, integer maps, masks, counts, outputs that are one
fp32 rounding of their inputs, zeros, untouched memory, sums whose order the kernel fixes.  No case excludes elements.  Output
buffers are allocated longer than needed and pre-filled with a NaN pattern no input produces (bytes 0xEF 0xBE 0xC0 0x7F for the
byte masks, 0x7FC0BEEF7FC0BEEF for the int64 lists); buffers a kernel adds into start from guarded zeros or known values.  The
cases are built in tests/_gen_kernel_refs.py, where tests/test_gen_kernel_refs_cpu.py asserts their preconditions without a GPU.
GSVC_PRINT_ERRORS=1 prints e_kernel and e32 of every case.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _gen_kernel_refs as G
from tests._gen_kernel_refs import err, ulp_distance
from tests.test_loss_kernels_gpu import SENTINEL, _i64, _lib, _rule, _sentinel, _sentinel_i32, _untouched, _written, _zeros_guarded

pytestmark = pytest.mark.gpu


def _cu(t):
    return None if t is None else t.cuda().contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _sentinel_i64(n):
    return _sentinel_i32(2 * n).view(torch.int64)


def _sentinel_u8(n):
    return _sentinel_i32((n + 3) // 4).view(torch.uint8)


def _u8_written(buf, n):
    """Bytes [0, n) hold only 0 and 1, every byte past n is the sentinel's."""
    return bool((buf[:n] <= 1).all()) and torch.equal(buf[n:], _sentinel_u8(n)[n:])


def _i64_written(buf, n):
    return _written(buf, 2 * n)


def _offset_bytes(t, offset):
    """The bytes of ``t`` at ``offset`` bytes inside a larger 16-byte aligned allocation."""
    big = torch.zeros(t.numel() + 48, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 16 == 0
    view = big[offset:offset + t.numel()]
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == offset % 16
    return view


# ================================================================================================================ embed_pe
def _embed_call(anchor, bounds, cam, R, F, rows, slack=0):
    lb, L, st = _lib()
    W2 = 2 * (2 * F + 1)
    pe = _sentinel(rows * W2 + slack)
    camv = (C.c_float * 16)(*([float(v) for v in cam] + [0.0] * (16 - len(cam)))[:16])
    rc = L.gsvc_embed_pe(lb.ptr(anchor) if anchor is not None and anchor.numel() else None, _i64(list(bounds) + [bounds[-1]] * 18), camv, R, F,
                         lb.ptr(pe), st)
    return rc, pe


@pytest.mark.parametrize("case", G.EMBED_CASES, ids=[c[0] for c in G.EMBED_CASES])
def test_embed_pe_against_float64(case):
    """gsvc_embed_pe: F in {1, 3, 16, 24} (256 / F rows per workgroup: 256, 85, 16, 10) x one render of 2 (256 / F) + 1 rows (a
    partial last workgroup), 4 renders with empty ones first / in the middle / last, 16 renders of 0 .. 3 rows (one workgroup spans
    all of them for F <= 11) and 16 mixed renders.  cam_z holds 0 and negative values, |xa| reaches 0.4 (argument 0.4 * 2^23 at
    F = 24).  Columns 0 (cam_z) and W (xa, ONE fp32 subtraction) bit for bit; the sin / cos columns by the rule at scale 1.
    measured on the MI355X, worst over the cases, kernel / fp32 statement: camera half 5.6e-8 / 5.6e-8, anchor half 6.4e-8 / 6.4e-8
    (both at F = 24; 0.09 of the bound).  The figures of the other entries are in DESIGN 4g."""
    lb, L, st = _lib()
    c = G.embed_case(case)
    F, R, rows = c["F"], c["R"], c["rows"]
    W = 2 * F + 1
    anchor, cam = _cu(c["anchor"]), c["cam"]
    rc, pe = _embed_call(anchor, c["bounds"], cam.tolist(), R, F, rows)
    lb.check(rc, "gsvc_embed_pe")
    assert _written(pe, rows * 2 * W)
    got = pe[:rows * 2 * W].view(rows, 2 * W)
    r64 = G.embed_pe_ref(anchor, cam, c["bounds"], F, torch.float64)
    r32 = G.embed_pe_ref(anchor, cam, c["bounds"], F, torch.float32)
    cz, xa = G.embed_xa(anchor, cam, c["bounds"])
    assert _same_bits(got[:, 0], cz) and _same_bits(got[:, W], xa)
    # the camera half is the same 2 F + 1 numbers for every row of a render
    _rule(f"embed_pe {c['id']} camera", err(got[:, 1:W], r64[:, 1:W], 1.0), err(r32[:, 1:W], r64[:, 1:W], 1.0))
    _rule(f"embed_pe {c['id']} anchor", err(got[:, W + 1:], r64[:, W + 1:], 1.0), err(r32[:, W + 1:], r64[:, W + 1:], 1.0))


def test_embed_pe_no_rows_and_refusals():
    """rows == 0 (with a NULL anchor): OK, nothing written.  F = 25, 17 renders, 0 renders: refused, nothing written."""
    lb, L, st = _lib()
    rc, pe = _embed_call(None, [0, 0, 0], [0.1, 0.2], 2, 16, 0, slack=256)
    lb.check(rc, "gsvc_embed_pe")
    torch.cuda.synchronize()
    assert _untouched(pe)
    lb.check(L.gsvc_embed_pe(None, _i64([0] * 18), (C.c_float * 16)(), 2, 16, None, st), "gsvc_embed_pe")          # pe NULL as well
    anchor = torch.rand(40, 3, device="cuda")
    for R, F in ((1, 25), (17, 16), (0, 16), (1, 0)):
        rc, pe = _embed_call(anchor, [0] + [40] * 17, [0.1] * 16, R, F, 40 * 2, slack=40 * 100)
        with pytest.raises(lb.GsvcError, match="embed_pe: bad arguments"):
            lb.check(rc, "gsvc_embed_pe")
        torch.cuda.synchronize()
        assert _untouched(pe)


# ================================================================================================================ gather rows
def _gather_fwd(c, d, decoded):
    lb, L, st = _lib()
    F, K, S, rows = c["F"], c["K"], c["S"], c["rows"]
    outs = [_sentinel(rows * w) for w in (F, 3 * K, S, K)]
    p = [lb.ptr(t) if t.numel() else None for t in d["params"]]
    o = [lb.ptr(t) if w else None for t, w in zip(outs, (F, 3 * K, S, K))]
    lb.check(L.gsvc_gather_rows_forward(p[0], p[1], p[2], p[3], lb.ptr(d["vis"]), rows, F, K, S, decoded, o[0], o[1], o[2], o[3], st),
             "gsvc_gather_rows_forward")
    for t, w in zip(outs, (F, 3 * K, S, K)):
        assert _written(t, rows * w)
    return [t[:rows * w].view(rows, w) for t, w in zip(outs, (F, 3 * K, S, K))]


def _gather_dev(c):
    return dict(vis=_cu(c["vis"]), params=[_cu(t) for t in c["params"]], grads=[_cu(t) for t in c["grads"]])


@pytest.mark.parametrize("decoded", [0, 1])
@pytest.mark.parametrize("rows", G.GATHER_ROWS)
@pytest.mark.parametrize("dims", G.GATHER_DIMS, ids=lambda d: "F%d-K%d-S%d" % d)
def test_gather_rows_forward_against_float64(dims, rows, decoded):
    """gsvc_gather_rows_forward: the group subsets of its two callers (features only; offsets, scaling and masks), all four groups
    and (3, 1, 1) (8 columns: fewer than the 32 lanes of a row), rows in {1, 7, 8, 9 (8 rows per workgroup), 1000}, vis with
    repeats and the rows 0 and A - 1, raw and decoded.  Features, offsets and every decoded output bit for bit; exp(scaling) by
    the rule relative to |ref|; the straight-through mask (h - s) + s within 1 ulp of the hard value h that the float64 sigmoid
    decides (the cases keep |sigmoid - 0.01| >= 1e-6, planted values at 3e-6 on either side)."""
    c = G.gather_case(*dims, rows)
    d = _gather_dev(c)
    got = _gather_fwd(c, d, decoded)
    r64 = G.gather_fwd_ref(d["params"], d["vis"], decoded, torch.float64)
    r32 = G.gather_fwd_ref(d["params"], d["vis"], decoded, torch.float32)
    assert _same_bits(got[0], d["params"][0][d["vis"]]) and _same_bits(got[1], d["params"][1][d["vis"]])
    if decoded:
        assert _same_bits(got[2], d["params"][2][d["vis"]]) and _same_bits(got[3], d["params"][3][d["vis"]])
        return
    _rule(f"gather_fwd {dims} rows={rows} scaling", err(got[2], r64[2], r64[2].abs()), err(r32[2], r64[2], r64[2].abs()))
    h = r64[3].float()
    assert int(ulp_distance(got[3], h).max()) <= 1 if h.numel() else True
    assert not got[3][h == 0].any()                              # (0 - s) + s is exactly 0


MASK_SETS = (0.0, 2.0, 4.0, 6.0, 8.0, 10.0, float("inf"))


def _mask_rule(tag, got, r64, r32, scale, m):
    """The rule for the raw mask group of a gather backward, [A, K] against the raw masks m [A, K], on the nested sets m <= t for t
    in MASK_SETS (the last one holds every element).  The factor s (1 - s) is formed in fp32 from s = 1 / (1 + expf(-m)); for
    m > 0 one unit in the last place of s (2^-24) is a fraction 2^-24 e^m of 1 - s: 4e-7 at m = 2, 1.8e-4 at m = 8, 0.25 and more
    from m = 15 on.  Taken over all elements at once, both errors are those of the few largest m, and the bound then allows every
    other element an error of its whole scale.  On the set m <= t the fp32 statement's error is about 2^-24 e^t, so a factor
    that is wrong by more than ~4 * 2^-24 e^t on any element with m <= t fails there (3e-6 at t = 2, 7e-4 at t = 8) while no
    element is left out of the last set."""
    for t in MASK_SETS:
        lo = m <= t
        _rule(f"{tag} mask(m<={t:g})", err(got[lo], r64[lo], scale[lo]), err(r32[lo], r64[lo], scale[lo]))


def _gather_bwd(c, d, decoded, no_grad=None, no_out=None):
    """One atomic backward on guarded zeros: the four dense tensors ([A, W]); group ``no_grad`` gets a NULL gradient, group
    ``no_out`` a NULL output."""
    lb, L, st = _lib()
    F, K, S, rows, A = c["F"], c["K"], c["S"], c["rows"], c["A"]
    widths = (F, 3 * K, S, K)
    outs = [_zeros_guarded(A * w) for w in widths]
    g = [lb.ptr(t) if (w and k != no_grad) else None for k, (t, w) in enumerate(zip(d["grads"], widths))]
    o = [lb.ptr(t) if (w and k != no_out) else None for k, (t, w) in enumerate(zip(outs, widths))]
    lb.check(L.gsvc_gather_rows_backward(lb.ptr(d["params"][2]) if S else None, lb.ptr(d["params"][3]) if K else None, lb.ptr(d["vis"]), rows, F, K, S,
                                         decoded, g[0], g[1], g[2], g[3], o[0], o[1], o[2], o[3], st), "gsvc_gather_rows_backward")
    torch.cuda.synchronize()
    for t, w in zip(outs, widths):
        assert _untouched(t[A * w:])
    return [t[:A * w].view(A, w) for t, w in zip(outs, widths)]


@pytest.mark.parametrize("decoded", [0, 1])
@pytest.mark.parametrize("rows", G.GATHER_ROWS)
@pytest.mark.parametrize("dims", G.GATHER_DIMS, ids=lambda d: "F%d-K%d-S%d" % d)
def test_gather_rows_backward_against_float64(dims, rows, decoded):
    """gsvc_gather_rows_backward (float atomics onto guarded zeros): the forward's shapes; with 1000 rows anchor 5 is hit by 200 of
    them, most by 0 .. 2.  Every element by the scatter-sum rule (scale: the sum of the |terms| that meet in it), anchors no row
    names exactly zero (their scale is 0).  The raw mask group's factor s (1 - s) loses up to a quarter of its value in fp32 where the
    raw mask is large and positive (1 - s cancels; the fp32 statement loses as much, so the rule over all elements holds with a
    large e32): that group passes the rule on every nested set m <= t of _mask_rule, each with the small e32 of its own
    elements.  Then every present group in turn with a NULL gradient (its buffer stays exactly zero, the others as before) and
    with a NULL output beside a present gradient."""
    c = G.gather_case(*dims, rows)
    d = _gather_dev(c)
    widths = (c["F"], 3 * c["K"], c["S"], c["K"])
    r64, sc = G.gather_bwd_ref(d["params"], d["vis"], d["grads"], decoded, torch.float64)
    r32, _ = G.gather_bwd_ref(d["params"], d["vis"], d["grads"], decoded, torch.float32)
    unnamed = torch.ones(c["A"], dtype=torch.bool, device="cuda")
    unnamed[d["vis"]] = False
    assert bool(unnamed.any())

    def check(got, skip, tag):
        for k, nm in enumerate(("feat", "offset", "scaling", "mask")):
            if not widths[k]:
                continue
            if k in skip:
                assert not _bits(got[k]).any(), (tag, nm)
                continue
            if k == 3 and not decoded:
                _mask_rule(f"gather_bwd {dims} rows={rows} dec={decoded} {tag}", got[k], r64[k], r32[k], sc[k], d["params"][3])
            else:
                _rule(f"gather_bwd {dims} rows={rows} dec={decoded} {tag} {nm}", err(got[k], r64[k], sc[k]), err(r32[k], r64[k], sc[k]))
            assert not _bits(got[k][unnamed]).any()

    check(_gather_bwd(c, d, decoded), (), "all")
    for k in range(4):
        if widths[k]:
            check(_gather_bwd(c, d, decoded, no_grad=k), (k,), f"grad{k}=NULL")
            check(_gather_bwd(c, d, decoded, no_out=k), (k,), f"out{k}=NULL")


# ================================================================================================================ ranked backward
def _ranked_call(c, d, decoded, R=None, absent=(), no_out=()):
    lb, L, st = _lib()
    F, K, S, A = c["F"], c["K"], c["S"], c["A"]
    R = c["R"] if R is None else R
    widths = (F, 3 * K, S, K)
    outs = [_sentinel(A * w) for w in widths]
    g = [lb.ptr(t) if (t.numel() and k not in absent) else None for k, t in enumerate(d["grads"])]
    if c["rows"] == 0:          # no row at all: the gradients are empty tensors; any valid pointer stands for them
        some = torch.zeros(1, device="cuda")
        g = [lb.ptr(some) if (w and k not in absent) else None for k, w in enumerate(widths)]
    # a group of width 0 (F, K or S == 0) is left out: NULL gradient, NULL output and, for the scaling / mask groups, NULL
    # parameters, as the entry's two callers pass them
    o = [lb.ptr(t) if (w and k not in no_out) else None for k, (t, w) in enumerate(zip(outs, widths))]
    rc = L.gsvc_gather_rows_backward_ranked(lb.ptr(d["params"][2]) if S else None, lb.ptr(d["params"][3]) if K else None,
                                            lb.ptr(d["seen"]) if c["R"] else None, lb.ptr(d["rank"]) if c["R"] else None, R, A, F, K, S,
                                            decoded, g[0], g[1], g[2], g[3], o[0], o[1], o[2], o[3], st)
    return rc, outs


RANKED_CASES = ([(R, A, p, G.RANKED_DIMS) for R in G.RANKED_R for A in G.RANKED_A for p in G.RANKED_PATTERNS[R]]
                + [(R, A, p, dims) for dims in G.RANKED_SUBSET_DIMS for R, A, p in G.RANKED_SUBSET_SHAPES])


@pytest.mark.parametrize("R,A,pattern,dims", RANKED_CASES,
                         ids=[f"R{R}-A{A}-{p}" + ("" if dims == G.RANKED_DIMS else "-F%d-K%d-S%d" % dims) for R, A, p, dims in RANKED_CASES])
def test_gather_rows_backward_ranked_exact_and_float64(R, A, pattern, dims):
    """gsvc_gather_rows_backward_ranked: R in {0, 1, 2, 8}, A in {1, 63, 64, 65 (64 anchors per workgroup), 1000}; views: one empty
    and one full, an anchor no view holds and one all 8 hold; all four groups (F, K, S) = (50, 10, 6), and at R A = 0 x 64, 1 x 63,
    2 x 65 and 8 x 1000 the subsets of the entry's two callers: (50, 0, 0) with scaling_p and mask_p NULL, and (0, 10, 6) (the
    groups left out get NULL gradients and outputs, and nothing is written for them).  Output buffers start as the sentinel:
    every element of a present group is written, a group whose gradient (or whose output) is NULL is NOT written (each in turn).
    Feature and offset groups bit-equal to the sequential fp32 sum in view order over 8 slots from 0.f (a column of -0.0 gradients
    comes out as +0.0); scaling and mask groups by the rule after the activation factor (scale: sum of |terms| times the factor),
    the mask group also on every set m <= t of _mask_rule; two runs give the same bits; raw and decoded."""
    lb, L, st = _lib()
    c = G.ranked_case(R, A, pattern, dims)
    d = dict(seen=_cu(c["seen"].to(torch.uint8).reshape(-1)), rank=_cu(c["rank"]), params=[_cu(t) for t in c["params"]],
             grads=[_cu(t) for t in c["grads"]])
    widths = (c["F"], 3 * c["K"], c["S"], c["K"])
    for decoded in (0, 1):
        rc, outs = _ranked_call(c, d, decoded)
        lb.check(rc, "gsvc_gather_rows_backward_ranked")
        assert all(_written(t, A * w) for t, w in zip(outs, widths))
        got = [t[:A * w].view(A, w) for t, w in zip(outs, widths)]
        r64, sc = G.ranked_bwd_ref(c, decoded, torch.float64, "cuda")
        r32, _ = G.ranked_bwd_ref(c, decoded, torch.float32, "cuda")
        for k in (0, 1) + ((2, 3) if decoded else ()):
            assert got[k].shape == r32[k].shape and _same_bits(got[k], r32[k]), (k, decoded)
        if c["rows"]:
            assert all(not _bits(got[k][:, 0]).any() for k in (0, 1) if widths[k])        # +0.0 from -0.0 terms
        if not decoded and widths[2]:
            tag = f"ranked R={R} A={A} {pattern} {dims}"
            _rule(f"{tag} scaling", err(got[2], r64[2], sc[2]), err(r32[2], r64[2], sc[2]))
            _mask_rule(tag, got[3], r64[3], r32[3], sc[3], d["params"][3])
        held = c["seen"].any(dim=0).cuda()
        assert all(not _bits(t[~held]).any() for t in got)
        rc, outs2 = _ranked_call(c, d, decoded)
        lb.check(rc, "gsvc_gather_rows_backward_ranked")
        assert all(_same_bits(a, b) for a, b in zip(outs, outs2))
        for k in range(4):
            if not widths[k]:
                continue
            rc, outs3 = _ranked_call(c, d, decoded, absent=(k,))
            lb.check(rc, "gsvc_gather_rows_backward_ranked")
            torch.cuda.synchronize()
            assert _untouched(outs3[k]) and all(_same_bits(outs3[j], outs[j]) for j in range(4) if j != k)
            rc, outs3 = _ranked_call(c, d, decoded, no_out=(k,))                  # a NULL output beside a present gradient
            lb.check(rc, "gsvc_gather_rows_backward_ranked")
            torch.cuda.synchronize()
            assert _untouched(outs3[k]) and all(_same_bits(outs3[j], outs[j]) for j in range(4) if j != k)


def test_gather_rows_backward_ranked_refuses_9_views():
    lb, L, st = _lib()
    c = G.ranked_case(8, 65, "none-all")
    d = dict(seen=_cu(torch.cat([c["seen"], c["seen"][:1]]).to(torch.uint8).reshape(-1)), rank=_cu(torch.cat([c["rank"], c["rank"][:65]])),
             params=[_cu(t) for t in c["params"]], grads=[_cu(t) for t in c["grads"]])
    rc, outs = _ranked_call(c, d, 0, R=9)
    with pytest.raises(lb.GsvcError, match="at most 8 views"):
        lb.check(rc, "gsvc_gather_rows_backward_ranked")
    torch.cuda.synchronize()
    assert all(_untouched(t) for t in outs)


# ================================================================================================================ plan masks
def _plan_masks_call(c, d, with_chosen, R=None):
    lb, L, st = _lib()
    A = c["A"]
    R = c["R"] if R is None else R
    views = [d["vis"][r % c["R"]] for r in range(max(R, 1))]
    ptrs = (C.c_void_p * len(views))(*[v.data_ptr() for v in views])
    M, present, chosen = _sentinel_u8(R * A), _sentinel_u8(A), _sentinel_u8(R * A)
    rc = L.gsvc_plan_masks(ptrs, R, A, lb.ptr(d["mask"]) if with_chosen else None, c["K"], c["decoded"], lb.ptr(d["u"]) if with_chosen else None,
                           c["rate"], lb.ptr(M), lb.ptr(present), lb.ptr(chosen) if with_chosen else None, st)
    return rc, M, present, chosen


@pytest.mark.parametrize("A", G.PLAN_A)
@pytest.mark.parametrize("R", G.PLAN_R)
def test_plan_masks_exact(R, A):
    """gsvc_plan_masks: R in {1, 4, 16}, A in {1, 255, 256, 257, 3000}, and inside K in {1, 10}, raw and decoded masks, the sample
    at rate 0.05 (u == rate planted on a visible live anchor: chosen; nextafter(rate, +inf): not chosen), at rate 0 with every
    third u exactly 0, and chosen == NULL (mask_raw and u NULL too: chosen's buffer untouched).  Raw masks take the two values
    logit(0.01) -+ 3e-4 only (|sigmoid - 0.01| ~ 3e-6: the float64 decision is the kernel's): for K = 10 a row holds both, or is
    below throughout (40 % of them, added so that raw rows that are not live occur), for K = 1 one of the two; decoded masks have
    all-zero rows (not live) and one-hot rows.  M, present and chosen bit for bit, holding only 0 and 1."""
    lb, L, st = _lib()
    for K in G.PLAN_K:
        for decoded in (0, 1):
            for rate0 in (False, True):
                c = G.plan_masks_case(R, A, K, decoded, rate0)
                d = dict(vis=_cu(c["vis"]), mask=_cu(c["mask"]), u=_cu(c["u"]))
                for with_chosen in (True, False):
                    rc, M, present, chosen = _plan_masks_call(c, d, with_chosen)
                    lb.check(rc, "gsvc_plan_masks")
                    wM, wP, wC = G.plan_masks_ref(d["vis"], d["mask"], d["u"], c["rate"], decoded, with_chosen)
                    assert _u8_written(M, R * A) and _u8_written(present, A)
                    assert torch.equal(M[:R * A], wM.reshape(-1)) and torch.equal(present[:A], wP)
                    if not with_chosen:
                        torch.cuda.synchronize()
                        assert _untouched(chosen.view(torch.int32))
                        continue
                    assert _u8_written(chosen, R * A) and torch.equal(chosen[:R * A], wC.reshape(-1)), (K, decoded, rate0)
                    if not rate0:
                        assert int(chosen[0]) == 1 and (R * A < 2 or int(chosen[1]) == 0)
                    elif R * A >= 256:
                        assert bool(chosen[:R * A].any()) and not bool(chosen[:R * A][d["u"].reshape(-1) > 0].any())


def test_plan_masks_no_anchors_and_17_views():
    """A == 0: OK, nothing written.  R = 17 and R = 0: refused, nothing written."""
    lb, L, st = _lib()
    c = G.plan_masks_case(16, 257, 10, 0)
    d = dict(vis=_cu(c["vis"]), mask=_cu(c["mask"]), u=_cu(c["u"]))
    c0 = dict(c, A=0)
    rc, M, present, chosen = _plan_masks_call(c0, d, True)
    lb.check(rc, "gsvc_plan_masks")
    torch.cuda.synchronize()
    assert all(_untouched(t.view(torch.int32)) for t in (M, present, chosen))
    for R in (17, 0):
        rc, M, present, chosen = _plan_masks_call(c, d, True, R=R)
        with pytest.raises(lb.GsvcError, match="at most 16 views"):
            lb.check(rc, "gsvc_plan_masks")
        torch.cuda.synchronize()
        assert all(_untouched(t.view(torch.int32)) for t in (M, present, chosen))


# ================================================================================================================ plan scans
def _plan_scans_call(c, M, chosen, present):
    lb, L, st = _lib()
    R, A = c["R"], c["A"]
    nb = int(L.gsvc_plan_scans_scratch_bytes(R, A))
    assert nb > 0 and nb % 4 == 0
    scratch = _sentinel_i32(nb // 4 + 2)[2:]               # (8 bytes in: the scratch holds int64 first, and stays 8-byte aligned)
    assert scratch.data_ptr() % 8 == 0
    bufs = dict(scan=_sentinel_i64(R * A), flat=_sentinel_i64(R * A), sel=_sentinel_i64(R * A), pos=_sentinel_i64(A), distinct=_sentinel_i64(A),
                counts=_sentinel_i64(R + 2))
    lb.check(L.gsvc_plan_scans(lb.ptr(M), lb.ptr(chosen), lb.ptr(present), R, A, lb.ptr(scratch), lb.ptr(bufs["scan"]), lb.ptr(bufs["flat"]),
                               lb.ptr(bufs["sel"]) if chosen is not None else None, lb.ptr(bufs["pos"]), lb.ptr(bufs["distinct"]),
                               lb.ptr(bufs["counts"]), st), "gsvc_plan_scans")
    torch.cuda.synchronize()
    assert _untouched(scratch[nb // 4:])
    return bufs


@pytest.mark.parametrize("offsets", G.SCAN_OFFSETS, ids=lambda o: "off-%d-%d-%d" % o)
@pytest.mark.parametrize("case", G.SCAN_SHAPES, ids=[c[0] for c in G.SCAN_SHAPES])
def test_plan_scans_exact_at_every_alignment(case, offsets):
    """gsvc_plan_scans with the view masks, chosen and present at byte offsets (0, 0, 0), (1, 8, 15), (8, 15, 1) and (15, 1, 8)
    inside larger allocations: offset 0 takes the 16-byte loads of ps_count16, every other offset its byte-wise path from the first
    element to the last.  Shapes: A = 1 (R = 1 and 3), R A = 15, R A = 4096 and 8192 with every byte set, 4101 (a chunk edge inside a
    view), 12 000, and empty masks; then the same with chosen == NULL (counts[R] == 0, sel_rows untouched).  scan, flat, sel_rows,
    pos, distinct and the R + 2 counts bit for bit; flat, sel_rows and distinct are written up to their counts and untouched behind.
    The masks hold 0 and 1 only: include/gsvc_hip.h states "view_masks [R, A] (bytes, 0 / 1)" for this entry, so other non-zero byte
    values are outside its contract and not run."""
    c = G.plan_scans_case(case)
    R, A = c["R"], c["A"]
    M, chosen, present = (_offset_bytes(_cu(c[k]), o) for k, o in zip(("M", "chosen", "present"), offsets))
    for with_chosen in (True, False):
        b = _plan_scans_call(c, M, chosen if with_chosen else None, present)
        scan, flat, sel, pos, distinct, counts = G.plan_scans_ref(M.view(R, A), chosen.view(R, A) if with_chosen else None, present)
        n_flat, n_dist = int(flat.numel()), int(distinct.numel())
        assert _i64_written(b["scan"], R * A) and torch.equal(b["scan"][:R * A], scan)
        assert _i64_written(b["flat"], n_flat) and torch.equal(b["flat"][:n_flat], flat)
        assert _i64_written(b["pos"], A) and torch.equal(b["pos"][:A], pos)
        assert _i64_written(b["distinct"], n_dist) and torch.equal(b["distinct"][:n_dist], distinct)
        assert _i64_written(b["counts"], R + 2) and torch.equal(b["counts"][:R + 2], counts)
        if with_chosen:
            assert _i64_written(b["sel"], int(sel.numel())) and torch.equal(b["sel"][:sel.numel()], sel)
            assert case[3] != "full" or int(counts[R]) == R * A
        else:
            assert int(b["counts"][R]) == 0 and _untouched(b["sel"])


# ================================================================================================================ compact by scan
@pytest.mark.parametrize("n", [0, 1, 256, 257, 5000])
def test_compact_by_scan_exact(n):
    """gsvc_compact_by_scan has no caller in the package (gsvc_plan_scans writes the step plan's lists itself); the entry is exported
    and declared, so it is held to its header: out[scan[i] - 1] = value ? value[i] + value_bias : i for every set mask[i].
    n in {0, 1, 256, 257, 5000}, random / empty / full masks, value NULL and present with a non-zero bias.  The prefix of `out`
    bit for bit, the tail untouched."""
    lb, L, st = _lib()
    gen = torch.Generator().manual_seed(n)
    for fill in ("random", "empty", "full"):
        mask = {"random": torch.rand(n, generator=gen) < 0.4, "empty": torch.zeros(n, dtype=torch.bool), "full": torch.ones(n, dtype=torch.bool)}[fill]
        mask = mask.to(torch.uint8).cuda()
        scan = torch.cumsum(mask.long(), 0)
        value = torch.randint(-1000, 1000, (n,), generator=gen).cuda()
        for val, bias in ((None, 0), (value, 0), (value, -12345)):
            out = _sentinel_i64(n)
            lb.check(L.gsvc_compact_by_scan(lb.ptr(mask) if n else None, lb.ptr(scan) if n else None, lb.ptr(val) if (n and val is not None) else None,
                                            bias, n, lb.ptr(out), st), "gsvc_compact_by_scan")
            want = G.compact_ref(mask, val, bias)
            assert _i64_written(out, int(want.numel())) and torch.equal(out[:want.numel()], want), (fill, bias)


# ================================================================================================================ context tail
@pytest.mark.parametrize("n,C", G.CTX_SHAPES)
def test_ctx_post_exact_gates_and_float64(n, C):
    """gsvc_ctx_post_forward / _backward: C in {1, 30}, n in {1, 9, 4097}; q holds exactly +-10, their outer fp32 neighbours and
    +-50, the scales exactly float32(1e-9), its lower neighbour, 0 and negative values.  Forward: mean and max(scale, 1e-9f) bit for
    bit, adj by the rule relative to |ref|.  Backward with all three gradients, each NULL in turn and all NULL: every element of
    dparams and dq written; [g_mean | g_scale where scale >= 1e-9f else 0] bit for bit; dq = g_adj * adj (ONE fp32 product of the
    forward's own adj: 0 ulp) where -10 <= q <= 10, exactly 0 outside; NULL slots exactly 0."""
    lb, L, st = _lib()
    c = G.ctx_post_case(n, C)
    d = {k: _cu(v) if torch.is_tensor(v) else v for k, v in c.items()}
    mean, scale, adj = _sentinel(n * C), _sentinel(n * C), _sentinel(n)
    lb.check(L.gsvc_ctx_post_forward(lb.ptr(d["params"]), lb.ptr(d["q"]), n, C, lb.ptr(mean), lb.ptr(scale), lb.ptr(adj), st), "gsvc_ctx_post_forward")
    assert _written(mean, n * C) and _written(scale, n * C) and _written(adj, n)
    m64, s64, a64 = G.ctx_post_fwd_ref(d["params"], d["q"], torch.float64)
    m32, s32, a32 = G.ctx_post_fwd_ref(d["params"], d["q"], torch.float32)
    assert _same_bits(mean[:n * C].view(n, C), m32) and _same_bits(scale[:n * C].view(n, C), s32)
    _rule(f"ctx_post n={n} C={C} adj", err(adj[:n], a64, a64.abs()), err(a32, a64, a64.abs()))
    sg, qg = G.ctx_post_gates(d["params"], d["q"])
    for use in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
        gm, gs, ga = (d[k] if u else None for k, u in zip(("g_mean", "g_scale", "g_adj"), use))
        dparams, dq = _sentinel(n * 2 * C), _sentinel(n)
        lb.check(L.gsvc_ctx_post_backward(lb.ptr(d["params"]), lb.ptr(d["q"]), lb.ptr(adj), n, C, lb.ptr(gm), lb.ptr(gs), lb.ptr(ga), lb.ptr(dparams),
                                          lb.ptr(dq), st), "gsvc_ctx_post_backward")
        assert _written(dparams, n * 2 * C) and _written(dq, n)
        wp, wq = G.ctx_post_bwd_ref(d["params"], d["q"], adj[:n], gm, gs, ga)
        gp, gq = dparams[:n * 2 * C].view(n, 2 * C), dq[:n]
        assert _same_bits(gp[:, :C], wp[:, :C]), use
        assert _same_bits(gp[:, C:], wp[:, C:]), use
        assert int(ulp_distance(gq, wq).max()) <= 0, use
        assert not _bits(gq[~qg]).any() and not _bits(gp[:, C:][~sg]).any()
        if use == (1, 1, 1):      # the planted boundary values pass, their outer neighbours do not
            for i, v in enumerate(c["q_plants"]):
                assert bool(gq[i] != 0) is (abs(v) == 10.0), (i, v)
            flat = gp[:, C:].reshape(-1)
            for i in range(c["ns"]):
                assert bool(flat[i] != 0) is (i == 0), i
        if use == (0, 0, 0):
            assert not _bits(gp).any() and not _bits(gq).any()


# ================================================================================================================ q rows
def _q_rows_bwd(c, d, present, D=None, rows=None):
    lb, L, st = _lib()
    D = c["D"] if D is None else D
    rows = c["rows"] if rows is None else rows
    out = _sentinel(3 * D)
    g = [lb.ptr(d["g"][k]) if present[k] else None for k in range(3)]
    a = [lb.ptr(d["adj"][k]) if c["raw"] else None for k in range(3)]          # read only when raw
    lb.check(L.gsvc_q_rows_backward(g[0], g[1], g[2], lb.ptr(d["ctx"]), *G.Q_BASE, rows, D, a[0], a[1], a[2], c["raw"], lb.ptr(out), st),
             "gsvc_q_rows_backward")
    return out


@pytest.mark.parametrize("raw", [0, 1])
@pytest.mark.parametrize("mapped,D", [(True, 1), (True, 700), (False, None)], ids=["D1", "D700", "no-map"])
@pytest.mark.parametrize("rows", G.Q_ROWS)
def test_q_rows_against_float64(rows, mapped, D, raw):
    """gsvc_q_rows_forward / _backward: rows in {1, 255, 257, 2500}, ctx_row onto D = 1 (every row on one slot), onto D = 700 (slot
    699 named by no row) and NULL (D = rows), raw in {0, 1}; the raw inputs hold exactly +-10, their outer neighbours and +-30.
    Forward: raw = 0 ONE fp32 product, bit for bit; raw = 1 by the rule relative to |ref|.  Backward into a sentinel-filled buffer
    (the zero fill is the entry's job): all 3 D elements written; with a map by the scatter-sum rule, slots no row names and
    slots whose every row lies outside the gate exactly 0 (their scale is 0); without a map raw = 0 bit for bit, raw = 1 by the
    rule on |term|; with all three gradients, and with one and with two of them NULL (those groups exactly 0)."""
    lb, L, st = _lib()
    c = G.q_rows_case(rows, D, mapped, raw)
    D = c["D"]
    d = dict(adj=_cu(c["adj"]), ctx=_cu(c["ctx"]), g=_cu(c["g"]))
    out = _sentinel(3 * rows)
    lb.check(L.gsvc_q_rows_forward(lb.ptr(d["adj"][0]), lb.ptr(d["adj"][1]), lb.ptr(d["adj"][2]), lb.ptr(d["ctx"]), *G.Q_BASE, rows, raw, lb.ptr(out),
                                   st), "gsvc_q_rows_forward")
    assert _written(out, 3 * rows)
    got = out[:3 * rows].view(3, rows)
    f64, f32 = G.q_rows_fwd_ref(d["adj"], d["ctx"], raw, torch.float64), G.q_rows_fwd_ref(d["adj"], d["ctx"], raw, torch.float32)
    tag = f"q_rows rows={rows} D={D} mapped={mapped} raw={raw}"
    if raw:
        _rule(f"{tag} forward", err(got, f64, f64.abs()), err(f32, f64, f64.abs()))
    else:
        assert _same_bits(got, f32)
    for present in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 1), (1, 0, 0)):
        buf = _q_rows_bwd(c, d, present)
        assert _written(buf, 3 * D)
        gb = buf[:3 * D].view(3, D)
        b64, sc = G.q_rows_bwd_ref(d["adj"], d["ctx"], raw, d["g"], present, torch.float64)
        b32, _ = G.q_rows_bwd_ref(d["adj"], d["ctx"], raw, d["g"], present, torch.float32)
        if not mapped and not raw:
            # 0 ulp, not the same bits: for a NULL group the statement's t * 0 is +-0.0 and the kernel writes +0.f, which the
            # check of the absent groups below pins bit for bit
            assert int(ulp_distance(gb, b32).max()) == 0, present
        else:
            _rule(f"{tag} backward {present}", err(gb, b64, sc), err(b32, b64, sc))
        for k in range(3):
            if not present[k]:
                assert not _bits(gb[k]).any()
        assert not gb[sc == 0].any()
        if mapped and D > 6:
            assert not _bits(gb[:, D - 1]).any()
        if raw and D >= 6 and rows >= 12 and present == (1, 1, 1):
            # slots 0 .. 5 hold the planted values (rotated by the group's number): +-10 pass, the others give exact zeros
            for k in range(3):
                vals = G.Q_PLANTS[k:] + G.Q_PLANTS[:k]
                for s, v in enumerate(vals):
                    assert bool(gb[k, s] != 0) is (abs(v) == 10.0), (k, s, v)


def test_q_rows_backward_no_slots_and_no_rows():
    """D == 0: OK, nothing written.  rows == 0 with D > 0 (under a map): the 3 D elements are zeroed, nothing past them."""
    c = G.q_rows_case(255, 700, True, 1)
    d = dict(adj=_cu(c["adj"]), ctx=_cu(c["ctx"]), g=_cu(c["g"]))
    buf = _q_rows_bwd(c, d, (1, 1, 1), D=0)
    torch.cuda.synchronize()
    assert _untouched(buf)
    buf = _q_rows_bwd(c, d, (1, 1, 1), rows=0)
    assert _written(buf, 3 * 700) and not _bits(buf[:3 * 700]).any()


# ================================================================================================================ segment rows sum
@pytest.mark.parametrize("kind", G.SEG_TARGETS)
@pytest.mark.parametrize("n", G.SEG_N)
@pytest.mark.parametrize("C_", G.SEG_C)
def test_segment_rows_sum_is_the_sequential_fp32_sum(C_, n, kind):
    """gsvc_segment_rows_sum: C in {1, 3, 50}, n in {1, 86 (86 * 3 = 258: a run head in a second workgroup), 1000}, targets all
    distinct, all equal (one run of n) and mixed (runs of ~8 on the even rows).  accumulate = 0 onto a sentinel-filled dst: the
    named rows are bit-equal to the sequential fp32 sum in list order from 0.f, every other row is untouched.  accumulate = 1
    onto known non-zero values: dst + acc with one fp32 add, other rows bit for bit as they were.  Two runs give the same bits."""
    lb, L, st = _lib()
    c = G.segment_case(n, C_, kind)
    T = c["T"]
    src, order, sidx = _cu(c["src"]), _cu(c["order"]), _cu(c["sorted_idx"])
    for accumulate in (0, 1):
        runs = []
        for _ in range(2):
            dst = _sentinel(T * C_)
            if accumulate:
                dst[:T * C_] = _cu(c["dst"]).reshape(-1)
            lb.check(L.gsvc_segment_rows_sum(lb.ptr(src), lb.ptr(order), lb.ptr(sidx), n, C_, lb.ptr(dst), accumulate, st), "gsvc_segment_rows_sum")
            torch.cuda.synchronize()
            assert _untouched(dst[T * C_:])
            runs.append(dst[:T * C_].view(T, C_).cpu())
        assert _same_bits(runs[0], runs[1])
        start = c["dst"].numpy() if accumulate else np.zeros((T, C_), dtype=np.float32)
        want, named = G.segment_rows_sum_f32(c, accumulate, start)
        got = runs[0].numpy()
        other = np.setdiff1d(np.arange(T), named)
        assert other.size > 0
        assert np.array_equal(got[named].view(np.int32), want[named].view(np.int32)), (accumulate, kind)
        if accumulate:
            assert np.array_equal(got[other].view(np.int32), start[other].view(np.int32))
        else:
            assert (got[other].view(np.int32) == SENTINEL).all()


# ================================================================================================================ film row maps
def _film_call(c, d, R=None):
    lb, L, st = _lib()
    R_ = c["R"] if R is None else R
    rows, D = c["rows"], c["D"]
    n_src = (c["R"] // 2) * D
    row_of, src_a, src_b = _sentinel_i32(rows), _sentinel_i32(n_src), _sentinel_i32(n_src)
    bounds = _i64(list(c["bounds"]) + [c["bounds"][-1]] * 20)
    p = lambda t: lb.ptr(t) if t.numel() else lb.ptr(d["M"])  # noqa: E731   (an empty list: any valid pointer)
    rc = L.gsvc_film_row_maps(p(d["vis"]), bounds, R_, lb.ptr(d["pos"]), D, c["A"], lb.ptr(d["M"]), lb.ptr(d["scan"]), p(d["distinct"]),
                              lb.ptr(row_of), lb.ptr(src_a), lb.ptr(src_b), st)
    return rc, row_of, src_a, src_b


@pytest.mark.parametrize("case", G.FILM_CASES, ids=[c[0] for c in G.FILM_CASES])
def test_film_row_maps_exact(case):
    """gsvc_film_row_maps: R in {2, 16}, A = 1, a pair of views both empty, an empty view opposite a full one, rows > (R / 2) D
    (R = 2, random) and rows < (R / 2) D (R = 16 with three views populated), all views empty (nothing written).  row_of, src_a
    and src_b bit for bit against the index statement, written in full and not past; every chain row appears exactly once among
    the non-negative src_a and src_b."""
    lb, L, st = _lib()
    c = G.film_case(case)
    d = {k: _cu(c[k]) for k in ("vis", "pos", "distinct", "scan")}
    d["M"] = _cu(c["M"].reshape(-1))
    rows, n_src = c["rows"], (c["R"] // 2) * c["D"]
    rc, row_of, src_a, src_b = _film_call(c, d)
    lb.check(rc, "gsvc_film_row_maps")
    assert _written(row_of, rows) and _written(src_a, n_src) and _written(src_b, n_src)
    w_row, w_a, w_b = (t.cuda() for t in G.film_row_maps_ref(c))
    assert torch.equal(row_of[:rows], w_row) and torch.equal(src_a[:n_src], w_a) and torch.equal(src_b[:n_src], w_b)
    named = torch.cat([src_a[:n_src], src_b[:n_src]])
    named = named[named >= 0].long()
    assert named.numel() == rows and torch.equal(torch.sort(named).values, torch.arange(rows, device="cuda"))
    if rows:
        # a chain row is one of the two sources of its FiLM row
        i = torch.arange(rows, device="cuda", dtype=torch.int32)
        assert bool(((src_a[:n_src][row_of[:rows].long()] == i) | (src_b[:n_src][row_of[:rows].long()] == i)).all())


def test_film_row_maps_refuses_odd_and_18_views():
    lb, L, st = _lib()
    c = G.film_case(G.FILM_CASES[2])
    d = {k: _cu(c[k]) for k in ("vis", "pos", "distinct", "scan")}
    d["M"] = _cu(c["M"].reshape(-1))
    for R in (3, 18, 0):
        rc, row_of, src_a, src_b = _film_call(c, d, R=R)
        with pytest.raises(lb.GsvcError, match="film_rows: an even number of views"):
            lb.check(rc, "gsvc_film_row_maps")
        torch.cuda.synchronize()
        assert _untouched(row_of) and _untouched(src_a) and _untouched(src_b)
