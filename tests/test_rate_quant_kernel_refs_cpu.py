"""The references of tests/_rate_quant_kernel_refs.py pinned on their own, without a GPU: a wrong reference must not be able to
bless a wrong kernel.  The sampled rate against a Python loop over rows with math.erf, the normalisation against the tensor
expression of test_rate_normalise_matches_tensor_expression, the exact STE statement against the torch CPU fp32 expression of
generate._seg_ste's tensor path, the table bits against train.get_binary_vxl_size_device in float64, every autograd gradient against
central differences in float64.  And the input builders of tests/test_rate_quant_kernels_gpu.py: every precondition that file relies
on is asserted here for every parametrised case, with the references alone.
"""
import math

import numpy as np
import pytest
import torch

from tests._rate_quant_kernel_refs import (LOW_BOUND, P_MAX32, P_MIN32, RN_CASES, RS_CASES, SPECIALS, STE_CASES, STE_Q_MODES, param_means_ref,
                                           rate_normalise_case, rate_normalise_coef, rate_normalise_ref, rate_sample_case,
                                           rate_sample_facts, rate_sample_loop, rate_sample_ref, render_of, ste_binary_bwd_ref,
                                           ste_binary_ref, ste_binary_table, quant_slab_sums_ref, ste_bounds_ref, ste_bounds_scalar_f32, ste_case, ste_fwd_f32,
                                           table_bits_f32, table_bits_ref, training_statis_ref)


def _rs_args(c, dtype=torch.float64):
    f = lambda t: None if t is None else t.to(dtype)  # noqa: E731
    return ([f(t) for t in c["x"]], [f(t) for t in c["mean"]], [f(t) for t in c["scale"]], [f(t) for t in c["Q"]], f(c["mask"]), c["sel"],
            c["sel_ctx"], f(c["x_mean"]), c["bounds"], c["K"])


# ------------------------------------------------------------------------------------------------------------ sampled rate
def test_render_of_rows():
    """Empty renders own no row; a row on a bound belongs to the render that starts there."""
    b = [0, 0, 4, 4, 9, 9]
    assert render_of(torch.arange(9), b).tolist() == [1, 1, 1, 1, 3, 3, 3, 3, 3]
    assert render_of(torch.arange(5), [0, 5]).tolist() == [0] * 5


@pytest.mark.parametrize("cid", ["n5-wide", "n5-c65", "n5-c130", "small-clamp", "small-low"])
def test_rate_sample_ref_against_a_loop_with_math_erf(cid):
    """Float64 rate_sample_ref = the row-by-row loop, to 1e-11 of each S: several renders (empty ones among them), distinct and
    repeated context rows, mask given and None, and small copies of the clamped and the floored case."""
    small = {"small-clamp": ("n40-clamp", 40, "wide", [50, 60], None, True, "clamp"),
             "small-low": ("n40-low", 40, "wide", [50, 0, 60], "repeat", False, "low")}
    case = small[cid] if cid in small else next(c for c in RS_CASES if c[0] == cid)
    c = rate_sample_case(case)
    S = rate_sample_ref(*_rs_args(c))
    L = lambda t: None if t is None else t.double().tolist()  # noqa: E731
    want = rate_sample_loop([L(t) for t in c["x"]], [L(t) for t in c["mean"]], [L(t) for t in c["scale"]], [L(t) for t in c["Q"]], L(c["mask"]),
                            c["sel"].tolist(), None if c["sel_ctx"] is None else c["sel_ctx"].tolist(), c["x_mean"].double().tolist(),
                            c["bounds"], c["K"])
    want = torch.tensor(want, dtype=torch.float64)
    assert S.shape == want.shape and bool((want.abs().sum(1) > 0).any())
    assert torch.allclose(S, want, rtol=1e-11, atol=0)
    if cid.startswith("small"):
        raws, margins, _ = rate_sample_facts(c)
        if cid == "small-clamp":
            assert bool((margins[1] < 0).any())
        else:
            assert any(bool((r < LOW_BOUND).any()) for r in raws)


def test_rate_sample_ref_gradients_against_central_differences():
    """Autograd of float64 rate_sample_ref w.r.t. x, mean, scale, Q and mask = central differences of sum(gS * S) (step 1e-6, to
    1e-6 of the largest entry), on a small case with three renders, repeated context rows and floored elements (all their gradients
    0).  The clamp bounds are constants of the statement, so the quotient is taken with the bounds of the unperturbed Q."""
    c = rate_sample_case(("n12-grad", 12, "one", [14, 0, 16], "repeat", True, "low"))
    args = _rs_args(c)
    gS = c["gS"].double()
    leaves = [[t.clone().requires_grad_(True) for t in grp] for grp in args[:4]]
    mask = args[4].clone().requires_grad_(True)
    S = rate_sample_ref(*leaves, mask, *args[5:])
    flat = [t for grp in leaves for t in grp] + [mask]
    grads = torch.autograd.grad((S * gS).sum(), flat)
    raws, _, _ = rate_sample_facts(c)
    assert any(bool((r < LOW_BOUND).any()) for r in raws)

    def value(vals):
        x, mean, scale, Q = (vals[0:3], vals[3:6], vals[6:9], vals[9:12])
        # Q enters twice: as the bin width (differentiated) and through the clamp bounds (constant) -> bounds from the original Q
        R = len(c["bounds"]) - 1
        from tests._rate_quant_kernel_refs import rate_bits_ref, rate_sample_bounds
        ctx = c["sel"] if c["sel_ctx"] is None else c["sel_ctx"]
        r = render_of(c["sel"], c["bounds"])
        tot = 0.0
        for g in range(3):
            lo, hi, _, _ = rate_sample_bounds(args[3][g], c["sel"], args[7][g], c["bounds"])
            bits, _ = rate_bits_ref(x[g][c["sel"]], mean[g][ctx], scale[g][ctx], Q[g][c["sel"]], lo, hi)
            if g == 2:
                bits = bits * vals[12][c["sel"]].repeat_interleave(3, dim=1)
            tot = tot + (torch.zeros(R, dtype=torch.float64).index_add(0, r, bits.sum(1)) * gS[:, g]).sum()
        return float(tot)

    base = [t.detach().clone() for t in flat]
    assert abs(value(base) - float((S.detach() * gS).sum())) <= 1e-12 * abs(float((S.detach() * gS).sum()))
    h = 1e-6
    for k, (t, g) in enumerate(zip(base, grads)):
        num = torch.zeros_like(t)
        for i in range(t.numel()):
            for sgn in (1, -1):
                v = [b.clone() for b in base]
                v[k].view(-1)[i] += sgn * h
                num.view(-1)[i] += sgn * value(v) / (2 * h)
        assert float((num - g).abs().max()) <= 1e-6 * max(float(g.abs().max()), 1.0), k
    # dense gradients: exactly zero at rows that were not selected
    unsel = torch.ones(c["rows"], dtype=torch.bool)
    unsel[c["sel"]] = False
    assert all(not grads[k][unsel].any() for k in (0, 1, 2, 9, 10, 11, 12))


@pytest.mark.parametrize("case", RS_CASES, ids=[c[0] for c in RS_CASES])
def test_rate_sample_cases_keep_away_from_every_decision(case):
    """The preconditions of the GPU file for every case: distinct sorted sel inside the rows; every element's float64 unfloored
    likelihood >= 2 LOW_BOUND or <= LOW_BOUND / 2; every x inside its clamp range by more than 1e-3 of the half-width or outside by
    as much; and the case has what its name promises (clamped fractions, floored fraction, an unsampled render, empty renders)."""
    c = rate_sample_case(case)
    sel = c["sel"]
    assert sel.numel() == c["n_sel"] == case[1] and sel.unique().numel() == sel.numel()
    assert sel.numel() == 0 or (int(sel.min()) >= 0 and int(sel.max()) < c["rows"] and bool((sel[1:] > sel[:-1]).all()))
    assert c["sel_ctx"] is None or (c["sel_ctx"].numel() == sel.numel() and int(c["sel_ctx"].max()) < c["ctx_rows"])
    assert 1 <= c["R"] <= 16 and c["bounds"][-1] == c["rows"]
    raws, margins, counts = rate_sample_facts(c)
    n_low = n_all = 0
    for g in range(3):
        assert bool(((raws[g] >= 2 * LOW_BOUND) | (raws[g] <= LOW_BOUND / 2)).all()), g
        assert bool((margins[g].abs() > 1e-3).all()), g
        n_low += int((raws[g] < LOW_BOUND).sum())
        n_all += raws[g].numel()
        if not (c["special"] == "clamp" and g == 1):
            assert bool((margins[g] > 0).all())
    if c["special"] == "clamp":
        lo_side = (c["x"][1][sel].double() < float(c["x_mean"][1])) & (margins[1] < 0)
        hi_side = (c["x"][1][sel].double() > float(c["x_mean"][1])) & (margins[1] < 0)
        assert 0.05 <= float(lo_side.double().mean()) <= 0.10 and 0.05 <= float(hi_side.double().mean()) <= 0.10
    if c["special"] == "low":
        assert 0.01 <= n_low / n_all <= 0.05
    else:
        assert n_low == 0
    if c["special"] == "unsampled":
        assert c["bounds"][2] - c["bounds"][1] > 0 and int(counts[1]) == 0 and c["R"] == 16
        assert c["bounds"][1] == c["bounds"][0] and c["bounds"][-1] == c["bounds"][-2]
    if case[4] == "three":
        assert c["sel_ctx"].unique().numel() <= 3
    assert bool((c["gS"].abs() >= 0.1).all())


def test_rate_sample_case_list_covers_the_issue():
    sizes = {c[1] for c in RS_CASES}
    assert sizes == {0, 1, 5, 4096, 4100, 9001, 16390}
    for cols in ("wide", "one", "c65", "c130"):
        assert {5, 4100} <= {c[1] for c in RS_CASES if c[2] == cols}
    assert {len(c[3]) if c[3] else 1 for c in RS_CASES} >= {1, 2, 16}
    assert any(c[4] is None for c in RS_CASES) and any(c[4] == "three" for c in RS_CASES) and any(c[4] == "repeat" for c in RS_CASES)
    assert any(not c[5] for c in RS_CASES) and any(c[5] for c in RS_CASES)
    assert {c[6] for c in RS_CASES} == {None, "clamp", "low", "unsampled"}


# ------------------------------------------------------------------------------------------------------------ normalisation
@pytest.mark.parametrize("case", RN_CASES, ids=[c[0] for c in RN_CASES])
def test_rate_normalise_ref_against_the_tensor_expression(case):
    """rate_normalise_ref in float64 = the expression of tests/test_grid_rate_gpu.py::test_rate_normalise_matches_tensor_expression
    (same NaN / inf pattern), its coef = keep rate / N, and autograd of out and sum = central differences.  The case builder: sel
    sorted and distinct, the render named unsampled has rows and no sampled one, every other render with rows is sampled."""
    c = rate_normalise_case(case)
    bounds, R, sel, om = c["bounds"], c["R"], c["sel"], c["om"].double()
    assert bool((sel[1:] > sel[:-1]).all()) and int(sel.max()) < c["rows"]
    S = c["S"].double().requires_grad_(True)
    out, total = rate_normalise_ref(S, om, sel, bounds, c["dims"])
    live = om.unsqueeze(2).sum(dim=1)[:, 0] > 0
    bt = torch.tensor(bounds)
    cnt = (bt[1:] - bt[:-1]).double()
    kr = torch.stack([live[bounds[r]:bounds[r + 1]].sum() for r in range(R)]).double() / cnt.clamp_min(1)
    edges = torch.searchsorted(sel, bt)
    ns = (edges[1:] - edges[:-1])
    N = ns.double().unsqueeze(1) * torch.tensor(c["dims"], dtype=torch.float64)
    per = S / N * kr.unsqueeze(1)
    tot = S.sum(dim=1) / N.sum(dim=1) * kr
    want = torch.cat([tot.unsqueeze(1), per], dim=1).detach()
    fin = torch.isfinite(want)
    assert torch.equal(fin, torch.isfinite(out)) and torch.equal(torch.isnan(want), torch.isnan(out))
    assert torch.equal(want[~fin & ~torch.isnan(want)], out[~fin & ~torch.isnan(out)])
    assert torch.allclose(out[fin], want[fin], rtol=1e-14, atol=0)
    ok = fin.all(dim=1)
    for r in range(R):
        rows_r = bounds[r + 1] - bounds[r]
        assert (int(ns[r]) == 0) == (rows_r == 0 or r == c["unsampled"])
        assert bool(ok[r]) == (int(ns[r]) > 0)
    if c["unsampled"] is not None:
        assert bounds[c["unsampled"] + 1] > bounds[c["unsampled"]]
        assert not math.isfinite(float(total.detach()))
    coef = rate_normalise_coef(S, om, sel, bounds, c["dims"])
    wantc = kr.unsqueeze(1) / torch.cat([N.sum(dim=1, keepdim=True), N], dim=1)
    assert torch.allclose(coef[ok], wantc[ok], rtol=1e-14, atol=0)
    for i in range(4):                      # the same numbers by autograd on the sampled renders
        (gi,) = torch.autograd.grad(out[ok][:, i].sum(), S, retain_graph=True)
        assert torch.allclose(gi[ok][:, max(i - 1, 0)], coef[ok][:, i], rtol=1e-14, atol=0)
    # gradient against central differences on the finite renders
    g_out, g_sum = c["g_out"].double(), float(c["g_sum"])

    def loss(Sv):
        o, _ = rate_normalise_ref(Sv, om, sel, bounds, c["dims"])
        return (o * g_out)[ok].sum() + g_sum * o[ok, 0].sum()

    (g,) = torch.autograd.grad(loss(S), S)
    h = 1e-3
    num = torch.zeros_like(g)
    for i in range(S.numel()):
        for sgn in (1, -1):
            Sv = S.detach().clone()
            Sv.view(-1)[i] += sgn * h
            num.view(-1)[i] += sgn * float(loss(Sv)) / (2 * h)
    assert float((num - g)[ok].abs().max()) <= 1e-7 * max(float(g[ok].abs().max()), 1e-30)


# ------------------------------------------------------------------------------------------------------------ means, statistics
def test_param_means_ref():
    gen = torch.Generator().manual_seed(4)
    f, s, o = (torch.randn(n, dtype=torch.float64, generator=gen) for n in (37, 11, 5))
    m, sc = param_means_ref(f, s, 1, o)
    assert abs(float(m[0]) - float(np.mean(f.numpy()))) < 1e-15 and abs(float(m[1]) - float(np.mean(np.exp(s.numpy())))) < 1e-15
    assert abs(float(m[2]) - float(np.mean(o.numpy()))) < 1e-15 and abs(float(sc[2]) - float(np.mean(np.abs(o.numpy())))) < 1e-15
    m0, _ = param_means_ref(f, s, 0, o[:0])
    assert abs(float(m0[1]) - float(np.mean(s.numpy()))) < 1e-15 and float(m0[2]) == 0.0


def test_training_statis_ref_against_a_loop():
    gen = torch.Generator().manual_seed(9)
    A, K, rows = 7, 3, 20
    vis = torch.randint(0, A, (rows,), generator=gen)
    op = torch.randn(rows * K, dtype=torch.float64, generator=gen)
    seen = torch.rand(rows * K, generator=gen) < 0.5
    grad = torch.randn(rows * K, 3, dtype=torch.float64, generator=gen)
    accs = [torch.rand(n, dtype=torch.float64, generator=gen) for n in (A, A, A * K, A * K)]
    out = training_statis_ref(vis, op, seen, grad, K, accs)
    want = [a.clone() for a in accs]
    for i in range(rows):
        a = int(vis[i])
        want[1][a] += 1
        for k in range(K):
            want[0][a] += max(float(op[i * K + k]), 0.0)
            if bool(seen[i * K + k]):
                want[2][a * K + k] += math.hypot(float(grad[i * K + k, 0]), float(grad[i * K + k, 1]))
                want[3][a * K + k] += 1
    assert all(torch.allclose(o, w, rtol=1e-14, atol=1e-14) for o, w in zip(out, want))


# ------------------------------------------------------------------------------------------------------------ STE quantiser
def _seg_ste_tensor_path(x, Q, offs, x_mean):
    """generate._seg_ste's tensor path (with _seg_bounds) on CPU fp32 tensors: per-row Q [rows, 1] or a number."""
    rows = x.shape[0]
    rr = torch.zeros(rows, dtype=torch.long)
    for r, (lo, hi) in enumerate(zip(offs[:-1], offs[1:])):
        rr[lo:hi] = r
    if torch.is_tensor(Q):
        R = len(offs) - 1
        cnt = torch.tensor([max(hi - lo, 1) for lo, hi in zip(offs[:-1], offs[1:])], dtype=torch.float32)
        qm = (torch.zeros(R).index_add_(0, rr, Q.reshape(-1)) / cnt)[rr].view(-1, 1)
    else:
        qm = Q
    centre = x_mean / qm
    lo, hi = centre - 15_000, centre + 15_000
    x1 = torch.clamp(x / Q, min=torch.trunc(torch.as_tensor(lo)), max=torch.trunc(torch.as_tensor(hi))) * Q
    return x1 + (torch.round(x1 / Q) * Q - x1)


@pytest.mark.parametrize("mode", list(STE_Q_MODES))
@pytest.mark.parametrize("case", STE_CASES, ids=[c[0] for c in STE_CASES])
def test_ste_statements_and_case_preconditions(case, mode):
    """ste_fwd_f32 (numpy, one operation at a time) = the torch CPU fp32 expression of _seg_ste's tensor path bit for bit, on the
    GPU file's own inputs and on random data with steps that are no powers of two; the float64 x_mean / qm -+ 15000 is further than
    1e-2 from an integer in every non-empty render, so the fp32 and float64 truncated bounds are the same integers; the data holds
    rows clamped on both sides, exact ties over odd and even k, and positive and negative quotients that round to 0."""
    c = ste_case(case, mode)
    per_row = c["per_row"]
    offs, x, Q = c["offs"], c["x"], c["Q"]
    q64 = Q.double() if per_row else float(Q[0])
    b64, raw64 = ste_bounds_ref(q64, c["x_mean"].double(), offs)
    live = torch.tensor([hi > lo for lo, hi in zip(offs[:-1], offs[1:])])
    assert bool(((raw64[live] - raw64[live].round()).abs() > 1e-2).all())
    b32, _ = ste_bounds_ref(Q if per_row else float(Q[0]), c["x_mean"], offs)
    assert torch.equal(b32[live].double(), b64[live])
    if not per_row:
        lo, hi = ste_bounds_scalar_f32(float(Q[0]), float(c["x_mean"]))
        assert bool((b32[:, 0] == float(lo)).all()) and bool((b32[:, 1] == float(hi)).all())
        assert not torch.isnan(b32).any()                     # a scalar step gives bounds to empty renders too
    else:
        assert torch.equal(torch.isnan(b32[:, 0]), ~live)
    bnd = torch.where(torch.isnan(b32), torch.zeros_like(b32), b32)
    y = ste_fwd_f32(x.numpy(), Q.numpy() if per_row else float(Q[0]), bnd.numpy(), offs)
    want = _seg_ste_tensor_path(x, Q.view(-1, 1) if per_row else float(Q[0]), offs, c["x_mean"])
    assert np.array_equal(y.view(np.int32), want.numpy().view(np.int32))
    # what the data holds
    qcol = Q.double().view(-1, 1)
    v = x.double() / qcol
    rr = torch.repeat_interleave(torch.arange(c["R"]), torch.tensor([b - a for a, b in zip(offs[:-1], offs[1:])]))
    lo64, hi64 = b64[rr, 0].view(-1, 1), b64[rr, 1].view(-1, 1)
    if max(b - a for a, b in zip(offs[:-1], offs[1:])) >= 63:
        assert bool((v > hi64).any()) and bool((v < lo64).any())
        ties = (v - v.floor() == 0.5) & torch.tensor(c["exact_ties"])
        assert not c["exact_ties"] or (bool((ties & (v.floor() % 2 == 0)).any()) and (c["C"] == 1 or bool((ties & (v.floor() % 2 == 1)).any())))
        yt = torch.from_numpy(y).double() / qcol
        assert bool((yt[ties] % 2 == 0).all())                          # ties went to the even neighbour
        zero = torch.from_numpy(y) == 0
        assert bool((zero & (x > 0)).any()) and (c["C"] == 1 or bool((zero & (x < 0)).any()))
        assert not bool(torch.signbit(torch.from_numpy(y)[zero]).any())           # x1 + (-0 Q - x1) = x1 + |x1| = +0
    # random steps that are no powers of two
    gen = torch.Generator().manual_seed(3 + c["C"])
    Qr = 0.05 + 0.2 * torch.rand(c["rows"], generator=gen)
    br, _ = ste_bounds_ref(Qr if per_row else 0.2, c["x_mean"], offs)
    br = torch.where(torch.isnan(br), torch.zeros_like(br), br)
    y2 = ste_fwd_f32(x.numpy(), Qr.numpy() if per_row else 0.2, br.numpy(), offs)
    want2 = _seg_ste_tensor_path(x, Qr.view(-1, 1) if per_row else 0.2, offs, c["x_mean"])
    assert np.array_equal(y2.view(np.int32), want2.numpy().view(np.int32))


def test_quant_slab_sums_ref_adds_up_to_the_render_sums():
    c = ste_case(STE_CASES[3], "rows")
    x, q, offs = c["x"].double(), c["Q"].double(), c["offs"]
    part, mag = quant_slab_sums_ref(x, q, offs)
    assert part.shape == (8, 4, 2) and bool((mag >= part.abs()).all())
    for r, (a, e) in enumerate(zip(offs[:-1], offs[1:])):
        assert abs(float(part[r, :, 0].sum()) - float(x[a:e].sum())) < 1e-9 and abs(float(part[r, :, 1].sum()) - float(q[a:e].sum())) < 1e-12
        assert int((part[r, :, 1] != 0).sum()) == (e - a + 63) // 64


def test_ste_fwd_f32_rounds_ties_to_even_where_float64_would_not():
    """Among the fp32 neighbours of 2.5 Q (Q = 0.3f) there is an x whose fp32 quotient x / Q rounds onto the tie 2.5 (the statement
    answers 2 Q) while the true quotient lies above the tie (a float64 run answers 3 Q): the expectation has to be the fp32 one."""
    q = np.float32(0.3)
    x = np.float32(2.5) * q
    found = 0
    for _ in range(4):
        x = np.nextafter(x, np.float32(-1))
    for _ in range(9):
        if np.float32(x / q) == np.float32(2.5) and float(x) / float(q) > 2.5:
            y = ste_fwd_f32(np.array([[x]], np.float32), float(q), np.array([[-100.0, 100.0]], np.float32), [0, 1])
            assert abs(float(y[0, 0]) - 2 * float(q)) < 1e-6 and round(float(x) / float(q)) == 3
            found += 1
        x = np.nextafter(x, np.float32(9))
    assert found >= 1


# ------------------------------------------------------------------------------------------------------------ STE binary, table bits
def test_ste_binary_refs_on_the_special_values():
    x = torch.tensor(SPECIALS)
    y, count = ste_binary_ref(x)
    #            +0  -0   1  -1  1+  1-  -1- -1+  sub -sub inf -inf nan
    assert y.tolist() == [1, 1, 1, -1, 1, 1, -1, -1, 1, -1, 1, -1, -1] and count == 7
    g = torch.arange(1.0, 14.0)
    gx = ste_binary_bwd_ref(x, g, 4.0)
    assert gx.tolist() == [3, 4, 5, 6, 0, 8, 0, 10, 11, 12, 0, 0, 0]
    assert ste_binary_bwd_ref(x, None, 4.0).tolist() == [2, 2, 2, 2, 0, 2, 0, 2, 2, 2, 0, 0, 0]
    for n in (1, 255, 4095, 4096, 4097, 12289, 65536, 65537):
        t = ste_binary_table(n, n)
        assert t.numel() == n and (n < 13 or bool(torch.isnan(t).any()))
    t = ste_binary_table(12289, 1)
    for e in (4096, 8192, 12288):
        assert bool(torch.isnan(t[e - 7:e + 7]).any()) and bool(torch.isinf(t[e - 7:e + 7]).any())


@pytest.mark.parametrize("total", [8, 2 ** 22, 2 ** 26 + 4])
def test_table_bits_ref_against_the_tensor_expression(total):
    """table_bits_ref = train.get_binary_vxl_size_device's expression in float64 (with the fp32 clamp constants), and its stated
    gradient = the central difference of the bits in ones where p is not clamped, and the partial derivative at fixed p where it is."""
    for ones in (0, 1, total // 2, total - 1, total):
        counts = torch.tensor([float(ones)], dtype=torch.float64)
        bits, grad = table_bits_ref(counts, total)
        o = torch.tensor(float(ones), dtype=torch.float64)
        p = torch.clamp(o / total, min=P_MIN32, max=P_MAX32)
        want = o * (-torch.log2(p)) + (total - o) * (-torch.log2(1 - p)) + 32
        assert float(bits) == float(want)
        f = lambda v: float(table_bits_ref(torch.tensor([v], dtype=torch.float64), total)[0])  # noqa: E731
        if P_MIN32 < ones / total < P_MAX32 and total > 8:
            h = max(1.0, total * 1e-6)
            assert abs((f(ones + h) - f(ones - h)) / (2 * h) - float(grad)) <= 1e-6 * max(abs(float(grad)), 1e-3)
        else:
            assert abs(float(grad) - float(torch.log2((1 - p) / p))) == 0.0
    b32, g32 = table_bits_f32(torch.tensor([3.0, 2.0]), 8)
    b64, g64 = table_bits_ref(torch.tensor([3.0, 2.0]), 8)
    assert b32.dtype == torch.float32 and abs(float(b32) - float(b64)) < 1e-5 and abs(float(g32) - float(g64)) < 1e-6
