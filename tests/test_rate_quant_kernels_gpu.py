"""The second half of csrc/rate.hip (gsvc_rate_sample_forward / _backward, gsvc_rate_normalise_forward / _backward, gsvc_param_means,
gsvc_training_statis) and of csrc/quant.hip (gsvc_ste_quant_forward, gsvc_ste_binary_count, _count_many, _backward_many,
gsvc_table_bits) called through their C entry points, each against the float64 run of its plain tensor statement in
tests/_rate_quant_kernel_refs.py.

Error rule: e_kernel <= 4 * e32 + 4 * eps32, both errors against the float64 reference on the scale the case names, e32 being the
error of the same reference function run in fp32 on the GPU on the same inputs (never the kernel's own output).  Exact compares
wherever an output is one fp32 rounding of its inputs, a count, or must be zero or untouched.  Output buffers are allocated longer
than needed and pre-filled with a NaN pattern no finite input produces; buffers a kernel adds into start from guarded zeros or known
values.  The cases and their inputs are built in tests/_rate_quant_kernel_refs.py, where tests/test_rate_quant_kernel_refs_cpu.py
asserts their preconditions (margins from every decision boundary, distinct sel) without a GPU.
GSVC_PRINT_ERRORS=1 prints e_kernel and e32 of every case.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests._rate_quant_kernel_refs import (EPS32, RN_CASES, RS_CASES, STE_CASES, STE_Q_MODES, err, err_each, param_means_ref, quant_slab_sums_ref,  # noqa: F401
                                           rate_normalise_case, rate_normalise_coef, rate_normalise_ref, rate_sample_case,
                                           rate_sample_facts, rate_sample_ref, ste_binary_bwd_ref, ste_binary_ref, ste_binary_table,
                                           ste_bounds_ref, ste_bounds_scalar_f32, ste_case, ste_fwd_f32, table_bits_f32, table_bits_ref,
                                           training_statis_ref, ulp_distance)
from tests.test_loss_kernels_gpu import _i64, _lib, _rule, _sentinel, _sentinel_i32, _untouched, _written, _zeros_guarded

pytestmark = pytest.mark.gpu


def _cu(t):
    return None if t is None else t.cuda().contiguous()


def _guard_ok(buf, n):
    """Nothing was written past n (for buffers a kernel fills only in part)."""
    return _untouched(buf[n:])


def _row_scale(ref):
    """The scale of a gradient tensor: per element the larger of |ref| and its row's largest |ref| (a vector is its own rows)."""
    a = ref.abs()
    return a if a.dim() == 1 else a.amax(dim=1, keepdim=True).expand_as(a)


# ================================================================================================================ sampled rate
def _rs_desc(c, d, renders=None, bounds=None):
    from gsvc_amd import _lib as lb
    desc = lb.RateSampleC()
    for g in range(3):
        desc.x[g], desc.mean[g], desc.scale[g], desc.Q[g] = (d[k][g].data_ptr() for k in ("x", "mean", "scale", "Q"))
        desc.C[g] = c["C"][g]
    desc.mask = None if d["mask"] is None else d["mask"].data_ptr()
    desc.sel = d["sel"].data_ptr() if c["n_sel"] else None
    desc.sel_ctx = d["sel_ctx"].data_ptr() if (d["sel_ctx"] is not None and c["n_sel"]) else None
    rb = _i64(c["bounds"] if bounds is None else bounds)
    desc.row_bounds = rb
    desc.x_mean = d["x_mean"].data_ptr()
    desc.K, desc.renders, desc.n_sel = c["K"], (c["R"] if renders is None else renders), c["n_sel"]
    return desc, rb


def _rs_run(c, d):
    """One forward and one backward call on guarded buffers: (S [R, 3], grads dict of dense tensors)."""
    lb, L, st = _lib()
    R, rows, ctx_rows, K = c["R"], c["rows"], c["ctx_rows"], c["K"]
    desc, rb = _rs_desc(c, d)
    ns = int(L.gsvc_rate_sample_scratch_floats(c["n_sel"]))
    scratch, S = _sentinel(ns), _sentinel(3 * R)
    lb.check(L.gsvc_rate_sample_forward(C.byref(desc), lb.ptr(scratch), lb.ptr(S), st), "gsvc_rate_sample_forward")
    assert _written(S, 3 * R) and _guard_ok(scratch, ns)
    bufs = dict(dx=[_zeros_guarded(rows * c["C"][g]) for g in range(3)], dmean=[_zeros_guarded(ctx_rows * c["C"][g]) for g in range(3)],
                dscale=[_zeros_guarded(ctx_rows * c["C"][g]) for g in range(3)], dQ=[_zeros_guarded(rows) for g in range(3)])
    dmask = None if d["mask"] is None else _zeros_guarded(rows * K)
    arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])  # noqa: E731
    lb.check(L.gsvc_rate_sample_backward(C.byref(desc), lb.ptr(scratch), lb.ptr(d["gS"]), arr(bufs["dx"]), arr(bufs["dmean"]),
                                         arr(bufs["dscale"]), arr(bufs["dQ"]), lb.ptr(dmask), st), "gsvc_rate_sample_backward")
    torch.cuda.synchronize()
    out = {}
    for k, n0 in (("dx", rows), ("dmean", ctx_rows), ("dscale", ctx_rows)):
        for g in range(3):
            n = n0 * c["C"][g]
            assert _guard_ok(bufs[k][g], n), (k, g)
            out[f"{k}{g}"] = bufs[k][g][:n].view(n0, c["C"][g])
    for g in range(3):
        assert _guard_ok(bufs["dQ"][g], rows)
        out[f"dQ{g}"] = bufs["dQ"][g][:rows]
    if dmask is not None:
        assert _guard_ok(dmask, rows * K)
        out["dmask"] = dmask[:rows * K].view(rows, K)
    return S[:3 * R].view(R, 3).clone(), out


def _rs_ref(c, d, dtype):
    """(S, grads dict) of the statement in ``dtype`` on the GPU, the gradients by autograd for upstream gS."""
    f = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    leaves = {k: [f(t).clone().requires_grad_(True) for t in d[k]] for k in ("x", "mean", "scale", "Q")}
    mask = None if d["mask"] is None else f(d["mask"]).clone().requires_grad_(True)
    S = rate_sample_ref(leaves["x"], leaves["mean"], leaves["scale"], leaves["Q"], mask, d["sel"], d["sel_ctx"], f(d["x_mean"]), c["bounds"], c["K"])
    flat = leaves["x"] + leaves["mean"] + leaves["scale"] + leaves["Q"] + ([mask] if mask is not None else [])
    names = [f"{k}{g}" for k in ("dx", "dmean", "dscale", "dQ") for g in range(3)] + (["dmask"] if mask is not None else [])
    if c["n_sel"]:
        grads = torch.autograd.grad((S * f(d["gS"])).sum(), flat, allow_unused=True)
        grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, flat)]
    else:
        grads = [torch.zeros_like(t) for t in flat]
    return S.detach(), dict(zip(names, grads))


@pytest.mark.parametrize("case", RS_CASES, ids=[c[0] for c in RS_CASES])
def test_rate_sample_against_float64(case):
    """gsvc_rate_sample_forward and _backward together, per case of RS_CASES: n_sel in {0, 1, 5, 4096 (one row per wave, the last
    size), 4100 (a second row for four waves, 1024 blocks + 1), 9001, 16390 (second trip of the statistics loop; a clamped case, where the
    value at the bound shows the mean step)}, columns (50, 6,
    30), (1, 1, 3), (65, 6, 3) and (130, 64, 66) (second and third trip of the column loop), 1 .. 16 renders with empty ones first,
    in the middle and last, a render with rows but no selected row (S exactly 0), sel_ctx NULL / distinct / repeated / three rows
    for all, mask NULL / 0-1, 5-10 % of the scaling group clamped on each side (dx exactly 0 there), a few per cent below the
    likelihood floor (dx exactly 0 there).  S on the scale of each |S|; every gradient on the scale of its row's largest |ref|, dQ
    per element; unselected rows of dx and dQ bit-for-bit the zeros they were; S, dx and dQ bit-identical over two runs.
    measured on the MI355X, largest over the cases, kernel / fp32 statement: S 1.7e-6 / 1.7e-6, dx 5.8e-4 / 5.8e-4, dmean 2.5e-3 /
    2.6e-3, dscale 4.8e-3 / 2.1e-3, dQ 1.1e-3 / 1.1e-3, dmask 2.3e-5 / 2.3e-5; the case nearest its bound is n16390-clamp dscale1,
    4.8e-3 / 1.6e-3 = 0.74 of it (the small-step group: x - mean is the difference of two numbers near 30)."""
    c = rate_sample_case(case)
    d = {k: ([_cu(t) for t in v] if isinstance(v, list) and k != "bounds" else _cu(v) if torch.is_tensor(v) else v) for k, v in c.items()}
    tag = f"rate_sample {c['id']}"
    S, got = _rs_run(c, d)
    S64, g64 = _rs_ref(c, d, torch.float64)
    S32, g32 = _rs_ref(c, d, torch.float32)
    assert bool(torch.isfinite(S).all()) and all(bool(torch.isfinite(v).all()) for v in got.values())
    _rule(f"{tag} S", err(S, S64, S64.abs()), err(S32, S64, S64.abs()))
    assert set(got) == set(g64)
    for k in got:
        sc = _row_scale(g64[k])
        _rule(f"{tag} {k}", err(got[k], g64[k], sc), err(g32[k], g64[k], sc))
    # rows that were not selected: untouched zeros, bit for bit
    unsel = torch.ones(c["rows"], dtype=torch.bool, device="cuda")
    unsel[d["sel"]] = False
    for g in range(3):
        assert not got[f"dx{g}"].view(torch.int32)[unsel].any() and not got[f"dQ{g}"].view(torch.int32)[unsel].any()
    if c["n_sel"]:
        assert c["special"] == "low" or all(bool(got[f"dQ{g}"][d["sel"]].ne(0).all()) for g in range(2))      # (group 2: a row's mask may be all 0)
    # renders without a selected row
    raws, margins, counts = rate_sample_facts(c)
    assert not S[(counts == 0).cuda()].view(torch.int32).any()
    if c["special"] == "unsampled":
        assert int(counts[1]) == 0 and c["bounds"][2] > c["bounds"][1]
    if c["special"] == "clamp":
        out_of_range = (margins[1] < 0).cuda()
        dxs = got["dx1"][d["sel"]]
        assert bool(out_of_range.any()) and not dxs[out_of_range].any() and bool(dxs[~out_of_range].ne(0).all())
        assert bool(got["dmean1"][d["sel"]][out_of_range].ne(0).all())          # evaluated at the clamped value, not dropped
    if c["special"] == "low":
        for g in range(3):
            low = (raws[g] < 2.0 ** -16).cuda()
            assert bool(low.any()) and not got[f"dx{g}"][d["sel"]][low].any() and not g64[f"dx{g}"][d["sel"]][low].any()
    # the same bits in a second run
    S2, got2 = _rs_run(c, d)
    assert torch.equal(S.view(torch.int32), S2.view(torch.int32))
    assert all(torch.equal(got[f"{k}{g}"].view(torch.int32), got2[f"{k}{g}"].view(torch.int32)) for k in ("dx", "dQ") for g in range(3))


def test_rate_sample_refuses_0_and_17_renders():
    lb, L, st = _lib()
    c = rate_sample_case(RS_CASES[2])
    d = {k: ([_cu(t) for t in v] if isinstance(v, list) and k != "bounds" else _cu(v) if torch.is_tensor(v) else v) for k, v in c.items()}
    ns = int(L.gsvc_rate_sample_scratch_floats(c["n_sel"]))
    for renders in (0, 17):
        desc, rb = _rs_desc(c, d, renders=renders, bounds=[0] * 17 + [c["rows"]])
        scratch, S, grad = _sentinel(ns), _sentinel(3 * 17), _sentinel(c["rows"] * 64)
        arr = (C.c_void_p * 3)(*[grad.data_ptr()] * 3)
        with pytest.raises(lb.GsvcError, match="rate_sample_forward: bad arguments"):
            lb.check(L.gsvc_rate_sample_forward(C.byref(desc), lb.ptr(scratch), lb.ptr(S), st), "gsvc_rate_sample_forward")
        with pytest.raises(lb.GsvcError, match="rate_sample_backward: bad arguments"):
            lb.check(L.gsvc_rate_sample_backward(C.byref(desc), lb.ptr(scratch), lb.ptr(d["gS"]), arr, arr, arr, arr, lb.ptr(grad), st),
                     "gsvc_rate_sample_backward")
        torch.cuda.synchronize()
        assert _untouched(scratch) and _untouched(S) and _untouched(grad)


# ================================================================================================================ normalisation
def _rn_forward(c, d, R=None):
    lb, L, st = _lib()
    R = c["R"] if R is None else R
    nb = int(L.gsvc_rate_normalise_scratch_bytes())
    scratch, out, coef, total = _sentinel_i32(nb // 4), _sentinel(4 * max(R, 1)), _sentinel(4 * max(R, 1)), _sentinel(1)
    dims = (C.c_float * 3)(*c["dims"])
    bounds = _i64(list(c["bounds"]) + [c["bounds"][-1]] * 18)
    rc = L.gsvc_rate_normalise_forward(lb.ptr(d["S"]), lb.ptr(d["om"]), c["K"], lb.ptr(d["sel"]), int(d["sel"].numel()), bounds, R, dims,
                                       lb.ptr(scratch), lb.ptr(out), lb.ptr(coef), lb.ptr(total), st)
    return rc, scratch, out, coef, total


def _same_pattern(got, ref):
    """NaN where the reference has NaN, the same infinity where it has one."""
    nan = torch.isnan(ref)
    inf = torch.isinf(ref)
    return torch.equal(torch.isnan(got), nan) and torch.equal(torch.isinf(got), inf) and torch.equal(got[inf].double(), ref[inf].double())


@pytest.mark.parametrize("case", RN_CASES, ids=[c[0] for c in RN_CASES])
def test_rate_normalise_against_float64(case):
    """gsvc_rate_normalise_forward and _backward: R in {1, 4, 16}, rows in {16 (fewer rows than the 256 counting blocks), 255, 257,
    5000} with render bounds inside a counting block's share, K in {1, 10}, renders of 0 and 1 rows, a render without sampled rows
    (the NaN / inf pattern of the reference in its four outputs, in coef and in the sum), all masks zero (every output exactly 0).
    out and coef on the scale of |ref| per entry, the sum on sum |out[:, 0]|; the backward from the kernel's own coef with g_out
    only, g_sum only and both, on the scale of the row's largest |ref|."""
    lb, L, st = _lib()
    c = rate_normalise_case(case)
    d = {k: _cu(v) if torch.is_tensor(v) else v for k, v in c.items()}
    R, tag = c["R"], f"rate_normalise {c['id']}"
    rc, scratch, out, coef, total = _rn_forward(c, d)
    lb.check(rc, "gsvc_rate_normalise_forward")
    assert _written(out, 4 * R) and _written(coef, 4 * R) and _written(total, 1) and _written(scratch, scratch.numel() - 8)
    out, coef = out[:4 * R].view(R, 4), coef[:4 * R].view(R, 4)
    o64, t64 = rate_normalise_ref(d["S"].double(), d["om"].double(), d["sel"], c["bounds"], c["dims"])
    o32, t32 = rate_normalise_ref(d["S"], d["om"], d["sel"], c["bounds"], c["dims"])
    c64 = rate_normalise_coef(d["S"].double(), d["om"].double(), d["sel"], c["bounds"], c["dims"])
    c32 = rate_normalise_coef(d["S"], d["om"], d["sel"], c["bounds"], c["dims"])
    ok = torch.isfinite(o64).all(dim=1)
    assert _same_pattern(out, o64) and _same_pattern(coef, c64) and _same_pattern(total[:1], t64.reshape(1))
    assert bool(ok.any()) and (c["unsampled"] is None or not bool(ok[c["unsampled"]]))
    _rule(f"{tag} out", err(out[ok], o64[ok], o64[ok].abs()), err(o32[ok], o64[ok], o64[ok].abs()))
    _rule(f"{tag} coef", err(coef[ok], c64[ok], c64[ok].abs()), err(c32[ok], c64[ok], c64[ok].abs()))
    if bool(ok.all()):
        sc = float(o64[:, 0].abs().sum())
        if sc > 0:
            _rule(f"{tag} sum", abs(float(total[0].double()) - float(t64)) / sc, abs(float(t32.double()) - float(t64)) / sc)
        else:
            assert float(total[0]) == 0.0 and not out.any()
    # backward
    for use_out, use_sum in ((True, False), (False, True), (True, True)):
        gS = _sentinel(3 * R)
        lb.check(L.gsvc_rate_normalise_backward(lb.ptr(coef), lb.ptr(d["g_out"]) if use_out else None, lb.ptr(d["g_sum"]) if use_sum else None,
                                                R, lb.ptr(gS), st), "gsvc_rate_normalise_backward")
        assert _written(gS, 3 * R)

        def grad(dtype):
            S = d["S"].to(dtype).clone().requires_grad_(True)
            o, _ = rate_normalise_ref(S, d["om"].to(dtype), d["sel"], c["bounds"], c["dims"])
            loss = (o * d["g_out"].to(dtype))[ok].sum() * float(use_out) + d["g_sum"].to(dtype)[0] * o[ok, 0].sum() * float(use_sum)
            return torch.autograd.grad(loss, S)[0]

        r64, r32 = grad(torch.float64), grad(torch.float32)
        sc = _row_scale(r64)[ok]
        _rule(f"{tag} gS out={use_out} sum={use_sum}", err(gS[:3 * R].view(R, 3)[ok], r64[ok], sc), err(r32[ok], r64[ok], sc))


def test_rate_normalise_refusals():
    lb, L, st = _lib()
    c = rate_normalise_case(RN_CASES[1])
    d = {k: _cu(v) if torch.is_tensor(v) else v for k, v in c.items()}
    for R in (0, 17):
        rc, scratch, out, coef, total = _rn_forward(c, d, R=R)
        with pytest.raises(lb.GsvcError, match="rate_normalise_forward: 1..16 renders, K > 0"):
            lb.check(rc, "gsvc_rate_normalise_forward")
        gS = _sentinel(64)
        with pytest.raises(lb.GsvcError, match="rate_normalise_backward: bad arguments"):
            lb.check(L.gsvc_rate_normalise_backward(lb.ptr(d["g_out"]), lb.ptr(d["g_out"]), None, R, lb.ptr(gS), st), "gsvc_rate_normalise_backward")
        torch.cuda.synchronize()
        assert all(_untouched(t) for t in (scratch, out, coef, total, gS))


# ================================================================================================================ parameter means
def _pm_call(tensors, scaling_exp):
    """tensors: three 1-D device tensors (views allowed: the pointer is the view's first element)."""
    lb, L, st = _lib()
    ns = int(L.gsvc_param_means_scratch_floats())
    scratch, out = _sentinel(ns), _sentinel(3)
    f, s, o = tensors
    p = lambda t: lb.ptr(t) if t.numel() else None  # noqa: E731
    lb.check(L.gsvc_param_means(p(f), f.numel(), p(s), s.numel(), scaling_exp, p(o), o.numel(), lb.ptr(scratch), lb.ptr(out), st),
             "gsvc_param_means")
    assert _written(out, 3) and _guard_ok(scratch, ns)
    return out[:3].clone()


def _pm_tensors(sizes, seed, shift=0):
    """randn (the scaling tensor 0.5 randn - 1, so that its exp is a sum of positive terms of mixed size), each in a buffer of its
    own; shift = 1 starts every tensor one float into its 16-byte aligned buffer."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for k, n in enumerate(sizes):
        buf = torch.empty(n + 4, device="cuda")
        v = torch.randn(n, device="cuda", generator=gen)
        buf[shift:shift + n] = 0.5 * v - 1 if k == 1 else v + 0.25
        assert buf.data_ptr() % 16 == 0
        out.append(buf[shift:shift + n])
    return out


PM_CASES = [("tails-1-2-3", (4001, 4002, 4003)), ("tails-3-1-2", (7, 1, 2)), ("no-feat", (0, 6001, 5003)), ("no-scaling", (5001, 0, 6003)),
            ("no-offset", (5001, 6002, 0)), ("only-scaling", (0, 4099, 0)), ("small-feat", (5000, 6000001, 5000002)),
            ("small-scaling", (6000001, 5000, 5000002)), ("small-offset", (6000001, 5000002, 5000)),
            ("anchors-100003", (100003 * 50, 100003 * 6, 100003 * 30))]


@pytest.mark.parametrize("scaling_exp", [0, 1])
@pytest.mark.parametrize("cid,sizes", PM_CASES, ids=[c[0] for c in PM_CASES])
def test_param_means_against_float64(cid, sizes, scaling_exp):
    """gsvc_param_means: lengths 1, 2 and 3 past a multiple of 4, each tensor empty in turn (its mean comes out as exactly 0: the
    sum over max(n, 1)), a 5000-element tensor in each position beside two large ones (11 000 003 in all: its share of the 2048
    workgroups rounds to 0 and it must still get one), the 100 003-anchor size (a trip of the four-deep loop), with and without
    exp.  Each mean on the scale of mean |term|; the same tensors one float into their buffers (the unaligned branch) against the
    same float64 value by the same rule; two runs bit-identical."""
    assert cid.startswith("small") is (min(sizes) == 5000 and sum(sizes) > 2048 * 5000)
    for shift in (0, 1):
        ts = _pm_tensors(sizes, 31 + len(cid), shift)
        assert all(t.data_ptr() % 16 == 4 * shift for t in ts if t.numel())
        got = _pm_call(ts, scaling_exp)
        m64, sc = param_means_ref(*(t.double() for t in ts[:2]), scaling_exp, ts[2].double())
        m32, _ = param_means_ref(ts[0], ts[1], scaling_exp, ts[2])
        for k, nm in enumerate(("feat", "scaling", "offset")):
            if sizes[k] == 0:
                assert float(got[k]) == 0.0 and not bool(torch.signbit(got[k]))
            else:
                s = float(sc[k])
                _rule(f"param_means {cid} exp={scaling_exp} shift={shift} {nm}", abs(float(got[k].double()) - float(m64[k])) / s,
                      abs(float(m32[k].double()) - float(m64[k])) / s)
        assert torch.equal(got.view(torch.int32), _pm_call(ts, scaling_exp).view(torch.int32))


def test_param_means_all_empty():
    """Three empty tensors (NULL pointers): 0, 0, 0."""
    e = torch.empty(0, device="cuda")
    got = _pm_call([e, e, e], 1)
    assert not got.view(torch.int32).any()


# ================================================================================================================ training statistics
ST_CASES = [("1x1", 1, 1, 2, 5), ("255x1", 255, 1, 3, 400), ("257x1", 257, 1, 2, 400), ("7001x10", 7001, 10, 3, 6000), ("26x10", 26, 10, 2, 30)]


def _statis_call(vis, op, seen, grad, stride, rows, K, accs, A):
    lb, L, st = _lib()
    bufs = []
    for a, n in zip(accs, (A, A, A * K, A * K)):
        b = _sentinel(n)
        b[:n] = a
        bufs.append(b)
    lb.check(L.gsvc_training_statis(lb.ptr(vis), lb.ptr(op), lb.ptr(seen), lb.ptr(grad), stride, rows, K, *(lb.ptr(b) for b in bufs), st),
             "gsvc_training_statis")
    assert all(_written(b, n) for b, n in zip(bufs, (A, A, A * K, A * K)))
    return [b[:n] for b, n in zip(bufs, (A, A, A * K, A * K))]


@pytest.mark.parametrize("cid,rows,K,stride,A", ST_CASES, ids=[c[0] for c in ST_CASES])
def test_training_statis_against_float64(cid, rows, K, stride, A):
    """gsvc_training_statis: rows K in {1, 255, 257, 70 010} (and 260 with K = 10), K in {1, 10}, grad rows 2 and 3 floats apart
    (the third never read: it holds NaN).  Only even anchors are visited: the odd ones keep their pre-filled values bit for bit.
    Counts exact; sums on the scale of the float64 sum (every term is >= 0) against the fp32 index_add statement."""
    gen = torch.Generator().manual_seed(rows + K)
    vis = _cu(2 * torch.randint(0, (A + 1) // 2, (rows,), generator=gen))
    op = _cu(torch.randn(rows * K, generator=gen))
    seen = _cu((torch.rand(rows * K, generator=gen) < 0.4).to(torch.uint8))
    grad = torch.randn(rows * K, stride, generator=gen)
    if stride > 2:
        grad[:, 2:] = float("nan")
    grad = _cu(grad)
    accs = [_cu(t) for t in (torch.rand(A, generator=gen), torch.full((A,), 3.0), torch.rand(A * K, generator=gen), torch.randint(0, 4, (A * K,), generator=gen).float())]
    got = _statis_call(vis, op, seen, grad, stride, rows, K, accs, A)
    r64 = training_statis_ref(vis, op.double(), seen, grad.double(), K, [a.double() for a in accs])
    r32 = training_statis_ref(vis, op, seen, grad, K, accs)
    assert torch.equal(got[1].double(), r64[1]) and torch.equal(got[3].double(), r64[3])
    for k, nm in ((0, "opacity_accum"), (2, "grad_accum")):
        _rule(f"training_statis {cid} {nm}", err(got[k], r64[k], r64[k].abs()), err(r32[k], r64[k], r64[k].abs()))
    odd = torch.arange(A, device="cuda") % 2 == 1
    oddk = odd.repeat_interleave(K)
    for k, m in ((0, odd), (1, odd), (2, oddk), (3, oddk)):
        assert torch.equal(got[k][m].view(torch.int32), accs[k][m].view(torch.int32))
    assert rows < 2 or bool((got[1][~odd] > 3).any())


def test_training_statis_2000_rows_on_one_anchor():
    """2000 rows all on anchor 3 (K = 10): 2000 atomic adds on one word and on each of its ten slots, in whatever order.  The inputs
    make every partial sum exact in fp32 (opacities are multiples of 1/1024 in [-1/2, 1/2], gradients (3, 4) m / 64 with integer
    m <= 32, whose norm 5 m / 64 is exact), so the result does not depend on the order and must equal the float64 one exactly."""
    rows, K, A = 2000, 10, 8
    gen = torch.Generator().manual_seed(2000)
    vis = torch.full((rows,), 3, dtype=torch.long).cuda()
    op = _cu(torch.randint(-512, 513, (rows * K,), generator=gen).float() / 1024)
    seen = _cu((torch.rand(rows * K, generator=gen) < 0.6).to(torch.uint8))
    m = torch.randint(0, 33, (rows * K, 1), generator=gen).float() / 64
    grad = _cu(torch.cat([3 * m, -4 * m], dim=1))
    accs = [_cu(t) for t in (torch.full((A,), 0.5), torch.full((A,), 3.0), torch.full((A * K,), 0.25), torch.zeros(A * K))]
    got = _statis_call(vis, op, seen, grad, 2, rows, K, accs, A)
    r64 = training_statis_ref(vis, op.double(), seen, grad.double(), K, [a.double() for a in accs])
    assert float(r64[0][3]) > 1000 and float(r64[2][30:40].min()) > 100 and float(r64[1][3]) == 2003.0
    assert all(torch.equal(g.double(), r) for g, r in zip(got, r64))


# ================================================================================================================ STE quantiser
def _ste_call(c, d, R=None):
    lb, L, st = _lib()
    R = c["R"] if R is None else R
    rows, Cq = c["rows"], c["C"]
    off = _i64(list(c["offs"]) + [c["offs"][-1]] * 10)
    ns = max(int(L.gsvc_noise_quant_scratch_floats(off, min(max(R, 1), 8))), 1)
    scratch, bounds, y = _sentinel(ns), _sentinel(2 * max(R, 1)), _sentinel(rows * Cq)
    q = d["Q"] if c["per_row"] else None
    rc = L.gsvc_ste_quant_forward(lb.ptr(d["x"]), lb.ptr(q), 0.0 if c["per_row"] else float(c["Q"][0]), lb.ptr(d["x_mean"]), off, R, Cq,
                                  lb.ptr(scratch), lb.ptr(bounds), lb.ptr(y), st)
    return rc, scratch, bounds, y, ns


@pytest.mark.parametrize("mode", list(STE_Q_MODES))
@pytest.mark.parametrize("case", STE_CASES, ids=[c[0] for c in STE_CASES])
def test_ste_quant_bit_for_bit(case, mode):
    """gsvc_ste_quant_forward: R in {1, 3, 8}, renders of 0, 1, 63, 64, 65 and 200 rows mixed, C in {1, 3, 50, 257}, a step per row
    (no powers of two but on the rows of ties) and one scalar step (1/8, and 0.2f).  Bounds: with per-row steps by the error rule against float64 on the scale of |ref| AND
    equal to the float64 ones as integers (x_mean / qm -+ 15000 is further than 1e-2 from an integer); with a scalar step bit for
    bit truncf(x_mean / q -+ 15000) in fp32, for empty renders too.  With per-row steps the scratch holds the sums of x and of the
    steps per 64-row slab of each render: by the rule, each on the sum of its absolute terms.  y: bit for bit ste_fwd_f32 given the kernel's own bounds; the
    data holds rows clamped on both sides, exact ties for odd and even k, positive and negative quotients that round to 0."""
    lb, L, st = _lib()
    c = ste_case(case, mode)
    per_row = c["per_row"]
    d = {k: _cu(v) if torch.is_tensor(v) else v for k, v in c.items()}
    R, rows, Cq, offs = c["R"], c["rows"], c["C"], c["offs"]
    rc, scratch, bounds, y, ns = _ste_call(c, d)
    lb.check(rc, "gsvc_ste_quant_forward")
    assert _written(bounds, 2 * R) and _written(y, rows * Cq)
    assert _written(scratch, ns) if per_row else _untouched(scratch)
    b = bounds[:2 * R].view(R, 2)
    live = torch.tensor([hi > lo for lo, hi in zip(offs[:-1], offs[1:])], device="cuda")
    if per_row:
        b64, _ = ste_bounds_ref(d["Q"].double(), d["x_mean"].double(), offs)
        b32, _ = ste_bounds_ref(d["Q"], d["x_mean"], offs)
        _rule(f"ste_quant {c['id']} bounds", err(b[live], b64[live], b64[live].abs()), err(b32[live], b64[live], b64[live].abs()))
        # the sums behind the step means, slab by slab (63, 64 and 65 rows: a partial slab, a full one, a full one and one row)
        p64, mag = quant_slab_sums_ref(d["x"].double(), d["Q"].double(), offs)
        p32, _ = quant_slab_sums_ref(d["x"], d["Q"], offs)
        assert p64.numel() == ns
        _rule(f"ste_quant {c['id']} slab sums", err(scratch[:ns].view(p64.shape), p64, mag), err(p32, p64, mag))
        assert torch.equal(b[live].double(), b64[live])
    else:
        lo, hi = ste_bounds_scalar_f32(float(c["Q"][0]), float(c["x_mean"]))
        want = torch.tensor([[lo, hi]] * R, dtype=torch.float32, device="cuda")
        assert torch.equal(b.view(torch.int32), want.view(torch.int32))
    bk = torch.where(live.view(-1, 1).expand(R, 2), b, torch.zeros_like(b)).cpu().numpy()
    want = ste_fwd_f32(c["x"].numpy(), c["Q"].numpy() if per_row else float(c["Q"][0]), bk, offs)
    gy = y[:rows * Cq].view(rows, Cq).cpu().numpy()
    diff = np.flatnonzero(gy.view(np.int32) != want.view(np.int32))
    assert diff.size == 0, (diff[:8], gy.reshape(-1)[diff[:8]], want.reshape(-1)[diff[:8]], c["x"].reshape(-1)[diff[:8]])
    if max(b - a for a, b in zip(offs[:-1], offs[1:])) >= 63:
        assert bool((want == 0).any())


def test_ste_quant_refuses_9_renders():
    lb, L, st = _lib()
    c = ste_case(STE_CASES[1], "rows")
    d = {k: _cu(v) if torch.is_tensor(v) else v for k, v in c.items()}
    for R in (0, 9):
        rc, scratch, bounds, y, _ = _ste_call(c, d, R=R)
        with pytest.raises(lb.GsvcError, match="ste_quant_forward: 1..8 renders, C > 0"):
            lb.check(rc, "gsvc_ste_quant_forward")
        torch.cuda.synchronize()
        assert _untouched(scratch) and _untouched(bounds) and _untouched(y)


# ================================================================================================================ STE binary
@pytest.mark.parametrize("n", [0, 1, 255, 65536, 65537])
def test_ste_binary_count_single_table(n):
    """gsvc_ste_binary_count: n in {0, 1, 255, 65 536 (256 blocks of 256 once), 65 537}; the special values (+-0, +-1 and their
    neighbours, the smallest subnormals, +-inf, NaN) by the predicate x >= 0; y and the count exact."""
    lb, L, st = _lib()
    x = ste_binary_table(n, 11 + n).cuda()
    y, count = _sentinel(n), _sentinel(1)
    lb.check(L.gsvc_ste_binary_count(lb.ptr(x) if n else None, n, lb.ptr(y) if n else None, lb.ptr(count), st), "gsvc_ste_binary_count")
    assert _written(y, n) and _written(count, 1)
    want, cnt = ste_binary_ref(x)
    assert torch.equal(y[:n].view(torch.int32), want.view(torch.int32)) and float(count[0]) == float(cnt)


STB_SIZES = {1: [[12289], [0]], 4: [[4096, 0, 4097, 1], [0, 4095, 0, 12289]], 8: [[0, 1, 4095, 0, 4096, 4097, 12289, 0]]}


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[None if (t is None or t.numel() == 0) else t.data_ptr() for t in ts])


@pytest.mark.parametrize("tables", [1, 4, 8])
def test_ste_binary_many_tables(tables):
    """gsvc_ste_binary_count_many and _backward_many: 1, 4 and 8 tables of 0, 1, 4095, 4096, 4097 and 12 289 entries with an empty
    table first, in the middle and last (NULL pointers), the special values around every 4096-entry chunk edge.  y, counts and the
    backward exact: grad_x = grad_y + count_grad / 2 where |x| <= 1 (one fp32 addition), with grad_y NULL for every second table,
    for all tables, with count_grads NULL, and with count_grads 1 and 2 floats apart."""
    lb, L, st = _lib()
    for sizes in STB_SIZES[tables]:
        xs = [ste_binary_table(n, 100 + 7 * k + n).cuda() for k, n in enumerate(sizes)]
        ys, counts = [_sentinel(n) for n in sizes], _sentinel(tables)
        lb.check(L.gsvc_ste_binary_count_many(_ptrs(xs), _ptrs([y if n else None for y, n in zip(ys, sizes)]), _i64(sizes), tables,
                                              lb.ptr(counts), st), "gsvc_ste_binary_count_many")
        assert _written(counts, tables) and all(_written(y, n) for y, n in zip(ys, sizes))
        for k, (x, y, n) in enumerate(zip(xs, ys, sizes)):
            want, cnt = ste_binary_ref(x)
            assert torch.equal(y[:n].view(torch.int32), want.view(torch.int32)) and float(counts[k]) == float(cnt), (sizes, k)
        gen = torch.Generator().manual_seed(sum(sizes))
        gys = [torch.randn(n, generator=gen).cuda() for n in sizes]
        cg = torch.randn(2 * tables, generator=gen).cuda()
        for g_mode, stride in (("all", 1), ("alternate", 2), ("none", 1), ("all", 0)):
            gy = [None if (g_mode == "none" or (g_mode == "alternate" and k % 2)) else g for k, g in enumerate(gys)]
            gxs = [_sentinel(n) for n in sizes]
            lb.check(L.gsvc_ste_binary_backward_many(_ptrs(xs), None if g_mode == "none" else _ptrs(gy), _i64(sizes), tables,
                                                     lb.ptr(cg) if stride else None, stride, _ptrs([g if n else None for g, n in zip(gxs, sizes)]),
                                                     st), "gsvc_ste_binary_backward_many")
            for k, (x, gx, n) in enumerate(zip(xs, gxs, sizes)):
                assert _written(gx, n)
                want = ste_binary_bwd_ref(x, gy[k], cg[k * stride] if stride else torch.zeros((), device="cuda"))
                assert torch.equal(gx[:n].view(torch.int32), want.view(torch.int32)), (sizes, g_mode, stride, k)


def test_ste_binary_many_refuses_0_and_9_tables():
    lb, L, st = _lib()
    xs = [torch.randn(16, device="cuda") for _ in range(9)]
    for tables in (0, 9):
        ys, counts = [_sentinel(16) for _ in range(9)], _sentinel(9)
        with pytest.raises(lb.GsvcError, match="ste_binary_count_many: 1..8 tables"):
            lb.check(L.gsvc_ste_binary_count_many(_ptrs(xs), _ptrs(ys), _i64([16] * 9), tables, lb.ptr(counts), st), "gsvc_ste_binary_count_many")
        with pytest.raises(lb.GsvcError, match="ste_binary_backward_many: 1..8 tables"):
            lb.check(L.gsvc_ste_binary_backward_many(_ptrs(xs), _ptrs(xs), _i64([16] * 9), tables, None, 0, _ptrs(ys), st),
                     "gsvc_ste_binary_backward_many")
        torch.cuda.synchronize()
        assert _untouched(counts) and all(_untouched(y) for y in ys)


# ================================================================================================================ table bits
@pytest.mark.parametrize("tables", [1, 8])
@pytest.mark.parametrize("total", [8, 2 ** 22, 2 ** 26 + 4])
def test_table_bits_against_float64(total, tables):
    """gsvc_table_bits from counts handed in directly: ones in {0, 1, total / 2, total - 1, total} dealt to 1 or 8 tables (each
    count rounded to fp32: the inputs are what the kernel is given; with 8 tables every count of these cases is exact), total in
    {8, 2^22, 2^26 + 4}: both clamped ends of p, p = 1/2 (gradient exactly 0), and a total that fp32 cannot hold.  out[0] on the scale
    of the sum of its absolute terms, out[1] on |log2 p| + |log2 (1 - p)|.
    This test found k_table_bits forming total - ones in float from a float total: with 2^26 + 3 ones of 2^26 + 4 the one zero was
    lost (bits 0.13 of their scale off; the fp32 statement with a float total as well, so it now keeps the counts as integers up
    to the formula).  The kernel now forms ones and total - ones in double, both exact, and rounds each once.
    measured on the MI355X, kernel / fp32 statement: bits 1.0e-2 / 1.0e-2 where p is clamped to 1e-6 (1 - p rounds in fp32),
    <= 9e-8 elsewhere, 9.7e-10 / 9.7e-10 at 2^26 + 3 of 2^26 + 4 in 8 tables; gradient 4.6e-8 / 8.6e-8."""
    lb, L, st = _lib()
    for ones in (0, 1, total // 2, total - 1, total):
        share = [ones // tables + (1 if k < ones % tables else 0) for k in range(tables)]
        counts = torch.tensor(share, dtype=torch.float64).float().cuda()
        assert tables == 1 or torch.equal(counts.double().cpu(), torch.tensor(share, dtype=torch.float64))
        out = _sentinel(2)
        lb.check(L.gsvc_table_bits(lb.ptr(counts), tables, total, lb.ptr(out), st), "gsvc_table_bits")
        assert _written(out, 2)
        b64, g64 = table_bits_ref(counts, total)
        b32, g32 = table_bits_f32(counts, total)
        n1 = float(counts.double().sum())
        p = min(max(n1 / total, float(np.float32(1e-6))), float(np.float32(1.0) - np.float32(1e-6)))
        s0 = n1 * abs(np.log2(p)) + (total - n1) * abs(np.log2(1 - p)) + 32
        s1 = abs(np.log2(p)) + abs(np.log2(1 - p))
        tag = f"table_bits total={total} tables={tables} ones={ones}"
        _rule(f"{tag} bits", abs(float(out[0].double()) - float(b64)) / s0, abs(float(b32.double()) - float(b64)) / s0)
        _rule(f"{tag} d bits / d ones", abs(float(out[1].double()) - float(g64)) / s1, abs(float(g32.double()) - float(g64)) / s1)
        if 2 * n1 == total:
            assert float(out[1]) == 0.0
