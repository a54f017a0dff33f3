"""tests/_gen_kernel_refs.py without a GPU: every statement is pinned against what the package already has on CPU tensors (the
embedders of gsvc_amd.time_util, the unfused branches of gsvc_amd.generate._gather_rows, cumsum / nonzero, index_add_), or, where
the package has neither an unfused path nor a CPU path, against float64 autograd of the forward statement or a plain Python loop;
and the preconditions of every case of tests/test_gen_kernels_gpu.py are asserted: the margin of every sigmoid > 0.01 decision,
the planted boundary values in the counts the cases name, index lists that are consistent and in range.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _gen_kernel_refs as G

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------- embed_pe
@pytest.mark.parametrize("case", G.EMBED_CASES, ids=[c[0] for c in G.EMBED_CASES])
def test_embed_statement_is_the_embedders_and_the_cases_reach_the_edges(case):
    from gsvc_amd.time_util import get_embedder
    c = G.embed_case(case)
    F, R, rows, counts = c["F"], c["R"], c["rows"], c["counts"]
    assert 1 <= F <= 24 and 1 <= R <= 16 and rows == sum(counts) and len(c["bounds"]) == R + 1
    rpb = 256 // F
    if case[2] == "one-partial":
        assert rows == 2 * rpb + 1 and rows % rpb == 1
    if case[2].startswith("four"):
        assert 0 in counts and (counts[0] == 0 or counts[-1] == 0) and 0 in counts[1:-1]
    if case[2] == "sixteen-tiny":
        assert R == 16 and max(counts) <= 3 and min(counts) == 0 and (rows <= rpb or F > 11)
    cam = c["cam"]
    assert R == 1 or (bool((cam == 0).any()) and bool((cam < 0).any()))
    cz, xa = G.embed_xa(c["anchor"], cam, c["bounds"])
    assert float(xa.abs().max()) >= 0.399 and float(xa.abs().max()) <= 0.401
    assert bool(torch.isnan(c["anchor"][:, :2]).all())                          # only z is read
    # the argument xa * 2^k is exact in fp32
    for k in range(F):
        assert torch.equal((xa * float(2 ** k)).double(), xa.double() * float(2 ** k))
    # rows of each render carry that render's camera
    want_cz = torch.cat([cam[r].repeat(n) for r, n in enumerate(counts)])
    assert torch.equal(cz, want_cz)
    embed, width = get_embedder(F, 1)
    assert width == 2 * F + 1
    want = torch.cat([embed(cz.double().unsqueeze(1)), embed(xa.double().unsqueeze(1))], dim=1)
    got = G.embed_pe_ref(c["anchor"], cam, c["bounds"], F, F64)
    assert got.shape == (rows, 2 * width) and float((got - want).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- gather
def _model(c, decoded, dtype=F64):
    f, o, s, m = (torch.nn.Parameter(p.to(dtype)) for p in c["params"])
    A, K = c["A"], c["K"]
    return SimpleNamespace(_anchor_feat=f, _offset=torch.nn.Parameter(o.detach().view(A, K, 3)), _scaling=s,
                           _mask=torch.nn.Parameter(m.detach().view(A, K, 1)), decoded_version=bool(decoded), scaling_activation=torch.exp)


def _package_gather(c, decoded, vis, grads):
    """Outputs and dense parameter gradients of the package's unfused branch (CPU tensors never take the fused one) in float64."""
    from gsvc_amd.generate import _gather_rows
    pc = _model(c, decoded)
    outs = _gather_rows(pc, vis)
    rows = vis.shape[0]
    flat = [o.reshape(rows, -1) for o in outs]
    sum((o * g.double()).sum() for o, g in zip(flat, grads)).backward()
    A = c["A"]
    return flat, [pc._anchor_feat.grad, pc._offset.grad.view(A, -1), pc._scaling.grad, pc._mask.grad.view(A, -1)]


@pytest.mark.parametrize("decoded", [0, 1])
@pytest.mark.parametrize("rows", G.GATHER_ROWS)
def test_gather_statements_are_the_unfused_branch(rows, decoded):
    c = G.gather_case(50, 10, 6, rows)
    outs, grads = _package_gather(c, decoded, c["vis"], c["grads"])
    ref = G.gather_fwd_ref(c["params"], c["vis"], decoded, F64)
    for a, b in zip(outs, ref):
        assert float((a.detach() - b).abs().max()) <= 1e-14
    gref, scale = G.gather_bwd_ref(c["params"], c["vis"], c["grads"], decoded, F64)
    for a, b, s in zip(grads, gref, scale):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(s.max()))
        assert not b[s == 0].any()


@pytest.mark.parametrize("dims", G.GATHER_DIMS, ids=lambda d: "F%d-K%d-S%d" % d)
@pytest.mark.parametrize("rows", G.GATHER_ROWS)
def test_gather_cases_meet_their_preconditions(dims, rows):
    c = G.gather_case(*dims, rows)
    F, K, S = dims
    vis, A = c["vis"], c["A"]
    assert vis.shape == (rows,) and int(vis.min()) >= 0 and int(vis.max()) < A and int(vis.max()) == A - 1
    if rows >= 7:
        assert int((vis == 0).sum()) >= 1 and int((vis == 1).sum()) >= 2                 # rows 0 and A - 1, a repeat
    if rows >= 1000:
        hits = torch.bincount(vis, minlength=A)
        assert int(hits[5]) >= 200 and float((hits <= 2).float().mean()) > 0.6 and int((hits == 0).sum()) > 0
    assert F + 3 * K + S + K > 0 and (dims != (3, 1, 1) or F + 3 * K + S + K < 32)
    mask = c["params"][3]
    if K:
        assert bool((G.sigmoid_margin(mask) >= G.MASK_MARGIN).all())                  # 100 % of the elements
        assert float(G.sigmoid_margin(mask[:2]).max()) < 1e-5                          # the planted pair, one on either side
        hard = G.ste_hard(mask)
        assert not bool(hard[0].any()) and bool(hard[1].all())
        assert rows < 7 or (bool(hard[vis].any()) and not bool(hard[vis].all()))         # both planted anchors are gathered


@pytest.mark.parametrize("R", G.RANKED_R)
@pytest.mark.parametrize("A", G.RANKED_A)
def test_ranked_statement_and_its_cases(R, A):
    for pattern in G.RANKED_PATTERNS[R]:
        c = G.ranked_case(R, A, pattern)
        seen, rank, vis, rows = c["seen"], c["rank"], c["vis"], c["rows"]
        assert seen.shape == (R, A) and rank.shape == (R * A,) and vis.shape == (rows,)
        # seen, rank and vis are consistent: rank - 1 at a seen (view, anchor) is the row that names that anchor
        flat = seen.reshape(-1)
        assert torch.equal(rank, torch.cumsum(flat.long(), 0)) and (rows == 0 or int(rank[-1]) == rows)
        j = flat.nonzero().squeeze(1)
        assert torch.equal(vis[rank[j] - 1], j % A) if rows else True
        if pattern == "empty-full":
            per_view = seen.sum(dim=1)
            assert int((per_view == 0).sum()) >= 1 and int((per_view == A).sum()) >= 1
        if pattern == "none-all":
            per_anchor = seen.sum(dim=0)
            assert int(per_anchor[A - 1]) == 8 and (A == 1 or int(per_anchor[0]) == 0)
        if c["K"]:
            assert bool((G.sigmoid_margin(c["params"][3]) >= G.MASK_MARGIN).all())
        for t in c["grads"][:2]:
            assert rows == 0 or bool(torch.signbit(t[:, 0]).all())
        for decoded in (0, 1):
            ref, scale = G.ranked_bwd_ref(c, decoded, F64)
            if rows:
                _, grads = _package_gather(c, decoded, vis, c["grads"])
            else:
                grads = [torch.zeros_like(r) for r in ref]
            for a, b, s in zip(grads, ref, scale):
                assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(s.max()))
        # the fp32 form is sequential in view order: it equals a per-element Python loop over the 8 slots
        if rows and A <= 65:
            acc, _ = G.ranked_sum(seen, rank, c["grads"][1], torch.float32)
            terms = G.ranked_view_terms(seen, rank, c["grads"][1], torch.float32).numpy()
            want = np.zeros(terms.shape[1:], dtype=np.float32)
            for v in range(8):
                want = want + terms[v]
            assert np.array_equal(acc.numpy().view(np.int32), want.view(np.int32))
            assert not acc[:, 0].view(torch.int32).any()                              # -0.0 terms: +0.0


@pytest.mark.parametrize("dims", G.RANKED_SUBSET_DIMS, ids=lambda d: "F%d-K%d-S%d" % d)
@pytest.mark.parametrize("R,A,pattern", G.RANKED_SUBSET_SHAPES)
def test_ranked_statement_on_the_callers_group_subsets(R, A, pattern, dims):
    """(F, 0, 0) and (0, K, S), the shapes of the entry's two callers: the statement against float64 autograd through the unfused
    branch of the same part of _gather_rows ("feat" / "rows"); the groups left out are empty."""
    from gsvc_amd.generate import _gather_rows
    c = G.ranked_case(R, A, pattern, dims)
    F, K, S = dims
    rows, vis = c["rows"], c["vis"]
    assert (c["F"], c["K"], c["S"]) == dims and [t.shape for t in c["grads"]] == [(rows, w) for w in (F, 3 * K, S, K)]
    assert [p.shape for p in c["params"]] == [(A, w) for w in (F, 3 * K, S, K)]
    assert torch.equal(c["rank"], torch.cumsum(c["seen"].reshape(-1).long(), 0)) and rows == int(c["seen"].sum())
    if K:
        assert bool((G.sigmoid_margin(c["params"][3]) >= G.MASK_MARGIN).all())
    for decoded in (0, 1):
        ref, scale = G.ranked_bwd_ref(c, decoded, F64)
        assert [r.shape for r in ref] == [(A, w) for w in (F, 3 * K, S, K)]
        if not rows:
            assert not any(bool(r.any()) for r in ref)
            continue
        pc = _model(c, decoded)
        outs = _gather_rows(pc, vis, parts="rows" if F == 0 else "feat")
        gin = c["grads"][1:] if F == 0 else c["grads"][:1]
        sum((o.reshape(rows, -1) * g.double()).sum() for o, g in zip(outs, gin)).backward()
        got = [pc._offset.grad.view(A, -1), pc._scaling.grad, pc._mask.grad.view(A, -1)] if F == 0 else [pc._anchor_feat.grad]
        want = ref[1:] if F == 0 else ref[:1]
        for a, b, s in zip(got, want, scale[1:] if F == 0 else scale[:1]):
            assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(s.max()))


# ---------------------------------------------------------------------------------------------------------------- plan masks
@pytest.mark.parametrize("R", G.PLAN_R)
@pytest.mark.parametrize("A", G.PLAN_A)
def test_plan_masks_statement_and_its_cases(R, A):
    rate32 = np.float32(G.PLAN_RATE)
    for K in G.PLAN_K:
        for decoded in (0, 1):
            for rate0 in (False, True):
                c = G.plan_masks_case(R, A, K, decoded, rate0)
                vis, mask, u = c["vis"], c["mask"], c["u"]
                assert vis.shape == (R, A) and mask.shape == (A, K) and u.shape == (R, A) and set(vis.unique().tolist()) <= {0, 1}
                if decoded:
                    assert set(mask.unique().tolist()) <= {0.0, 1.0}
                    if A >= 255:
                        s = mask.sum(dim=1)
                        assert int((s == 0).sum()) > 0 and int((s == 1).sum()) > 0
                else:
                    assert bool((G.sigmoid_margin(mask) >= G.MASK_MARGIN).all()) and float(G.sigmoid_margin(mask).max()) < 1e-5
                    assert mask.unique().numel() <= 2
                    if A >= 255:
                        assert mask.unique().numel() == 2
                    # every row holds a value on either side of the threshold (K >= 2) or is below throughout (the rows that are
                    # not live); both kinds occur
                    above = mask > G.LOGIT_001
                    both, dead = above.any(dim=1) & ~above.all(dim=1), ~above.any(dim=1)
                    assert bool((both | dead).all()) if K >= 2 else not bool(both.any())
                    if A >= 255:
                        assert int(dead.sum()) > 0 and int((~dead).sum()) > 0 and (K < 2 or int(both.sum()) > 0)
                M, present, chosen = G.plan_masks_ref(vis, mask, u, c["rate"], decoded)
                flat_u = u.view(-1)
                if rate0:
                    assert c["rate"] == 0.0 and int((flat_u == 0).sum()) == (R * A + 2) // 3
                else:
                    assert int((flat_u.numpy() == rate32).sum()) == 1 and float(flat_u[0]) == float(rate32) and int(chosen.view(-1)[0]) == 1
                    if R * A >= 2:
                        assert flat_u.numpy()[1] == np.nextafter(rate32, np.float32(np.inf)) and int(chosen.view(-1)[1]) == 0
                        assert int(M.view(-1)[1]) == 1
                # an independent statement, anchor by anchor
                if A <= 257 and R <= 4:
                    live = [(sum(float(v) for v in mask[a]) > 0) if decoded else any(1.0 / (1.0 + np.exp(-float(v))) > 0.01 for v in mask[a])
                            for a in range(A)]
                    for r in range(R):
                        for a in range(A):
                            v = bool(vis[r, a])
                            assert bool(M[r, a]) is v
                            assert bool(chosen[r, a]) is (v and live[a] and bool(u.numpy()[r, a] <= np.float32(c["rate"])))
                    assert all(bool(present[a]) is bool(vis[:, a].any()) for a in range(A))
                assert G.plan_masks_ref(vis, mask, u, c["rate"], decoded, with_chosen=False)[2] is None


# ---------------------------------------------------------------------------------------------------------------- scans
@pytest.mark.parametrize("case", G.SCAN_SHAPES, ids=[c[0] for c in G.SCAN_SHAPES])
def test_plan_scans_statement_and_its_cases(case):
    c = G.plan_scans_case(case)
    R, A, M, chosen, present = c["R"], c["A"], c["M"], c["chosen"], c["present"]
    assert set(M.unique().tolist()) <= {0, 1} and bool((chosen <= M).all()) and torch.equal(present, M.any(dim=0).to(torch.uint8))
    if case[3] == "full":
        assert bool(M.all()) and bool(chosen.all()) and (A == 1 or (R * A) % 4096 == 0)
    if case[0] == "below-16":
        assert R * A < 16
    scan, flat, sel, pos, distinct, counts = G.plan_scans_ref(M, chosen, present)
    # plain loops
    run, w_scan, w_flat, w_sel = 0, [], [], []
    for i, (m, ch) in enumerate(zip(M.reshape(-1).tolist(), chosen.reshape(-1).tolist())):
        run += m
        w_scan.append(run)
        if m:
            w_flat.append(i % A)
        if ch:
            w_sel.append(run - 1)
    assert scan.tolist() == w_scan and flat.tolist() == w_flat and sel.tolist() == w_sel
    run, w_pos, w_dist = 0, [], []
    for a, p in enumerate(present.tolist()):
        run += p
        w_pos.append(run - 1)
        if p:
            w_dist.append(a)
    assert pos.tolist() == w_pos and distinct.tolist() == w_dist
    assert counts.tolist() == [w_scan[(r + 1) * A - 1] for r in range(R)] + [len(w_sel), len(w_dist)]
    assert G.plan_scans_ref(M, None, present)[2] is None and int(G.plan_scans_ref(M, None, present)[5][R]) == 0
    # the lists are consistent: pos inverts distinct, the views' lists are ascending
    assert torch.equal(pos[distinct], torch.arange(distinct.numel()))
    # compaction by scan is nonzero
    value = torch.arange(R * A) * 3
    assert torch.equal(G.compact_ref(M.reshape(-1), None, 0), M.reshape(-1).nonzero().squeeze(1))
    assert torch.equal(G.compact_ref(M.reshape(-1), value, -7), value[M.reshape(-1) != 0] - 7)


# ---------------------------------------------------------------------------------------------------------------- context tail
@pytest.mark.parametrize("n,C", G.CTX_SHAPES)
def test_ctx_post_statement_is_float64_autograd_and_the_values_are_planted(n, C):
    c = G.ctx_post_case(n, C)
    params, q = c["params"], c["q"]
    assert c["nq"] == min(n, 6) if (n > 1 or C == 1) else c["nq"] == 1
    assert c["ns"] == min(n * C, 5)
    qn = q.numpy()
    if n >= 6:
        for v in (10.0, -10.0, 50.0, -50.0, np.nextafter(np.float32(10), np.float32(np.inf)), np.nextafter(np.float32(-10), np.float32(-np.inf))):
            assert int((qn == np.float32(v)).sum()) >= 1
        assert np.nextafter(np.float32(10), np.float32(np.inf)) > np.float32(10)
    else:
        assert abs(float(q[0])) == 10.0
    sc = params[:, C:].reshape(-1).numpy()
    assert sc[0] == np.float32(1e-9)
    if n * C >= 5:
        assert sc[1] == np.nextafter(np.float32(1e-9), np.float32(0)) and sc[1] < sc[0] and sc[2] == 0 and sc[3] < 0 and sc[4] == -sc[0]
    sg, qg = G.ctx_post_gates(params, q)
    assert bool(sg.reshape(-1)[0]) and (n * C < 5 or not bool(sg.reshape(-1)[1:5].any()))
    assert [bool(v) for v in qg[:c["nq"]]] == [abs(v) == 10.0 for v in c["q_plants"]]
    # float64 autograd of the forward statement written with torch's own clamp (whose gradient passes at the bounds)
    p64, q64 = params.double().requires_grad_(True), q.double().requires_grad_(True)
    mean, scale = p64[:, :C], torch.clamp(p64[:, C:], min=float(np.float32(1e-9)))
    adj = torch.exp(torch.clamp(q64, min=-10, max=10))
    rm, rs, ra = G.ctx_post_fwd_ref(params, q, F64)
    assert torch.equal(mean.detach(), rm) and torch.equal(scale.detach(), rs) and torch.equal(adj.detach(), ra)
    ((mean * c["g_mean"]).sum() + (scale * c["g_scale"]).sum() + (adj * c["g_adj"]).sum()).backward()
    adj32 = ra.float()
    wp, wq = G.ctx_post_bwd_ref(params, q, adj32, c["g_mean"], c["g_scale"], c["g_adj"])
    assert torch.equal(wp.double(), p64.grad)
    assert float((wq.double() - q64.grad).abs().max()) <= 1e-6 * float(q64.grad.abs().max())
    assert torch.equal(wq == 0, q64.grad == 0)
    zp, zq = G.ctx_post_bwd_ref(params, q, adj32, None, None, None)
    assert not zp.any() and not zq.any()
    hp, hq = G.ctx_post_bwd_ref(params, q, adj32, c["g_mean"], None, c["g_adj"])
    assert torch.equal(hp[:, :C], c["g_mean"]) and not hp[:, C:].any() and torch.equal(hq, wq)


# ---------------------------------------------------------------------------------------------------------------- q rows
@pytest.mark.parametrize("raw", [0, 1])
@pytest.mark.parametrize("mapped,D", [(True, 1), (True, 700), (False, None)], ids=["D1", "D700", "no-map"])
@pytest.mark.parametrize("rows", G.Q_ROWS)
def test_q_rows_statement_is_float64_autograd(rows, mapped, D, raw):
    c = G.q_rows_case(rows, D, mapped, raw)
    D, adj, ctx, g = c["D"], c["adj"], c["ctx"], c["g"]
    assert adj.shape == (3, D) and g.shape == (3, rows)
    if mapped:
        assert ctx.shape == (rows,) and int(ctx.min()) >= 0 and int(ctx.max()) < D
        if D > 6:
            assert not bool((ctx == D - 1).any()) and (rows < 12 or all(bool((ctx == s).any()) for s in range(6)))
    else:
        assert ctx is None and D == rows
    if raw and D >= 6:
        an = adj.numpy()
        for k in range(3):
            assert sorted(an[k, :6].tolist()) == sorted(float(np.float32(v)) for v in G.Q_PLANTS)
        assert {abs(v) for v in G.Q_PLANTS} == {10.0, float(np.nextafter(np.float32(10), np.float32(np.inf))), 30.0}
    a64 = adj.double().requires_grad_(True)
    qb = torch.tensor(G.Q_BASE, dtype=F64).view(3, 1)
    val = torch.exp(torch.clamp(a64, min=-10, max=10)) if raw else a64
    out = qb * (val if ctx is None else val[:, ctx])
    assert float((out.detach() - G.q_rows_fwd_ref(adj, ctx, raw, F64)).abs().max()) <= 1e-12 * float(out.detach().abs().max())
    for present in ((1, 1, 1), (0, 1, 1), (1, 0, 0)):
        w = g.double() * torch.tensor(present, dtype=F64).view(3, 1)
        grad, = torch.autograd.grad((out * w).sum(), a64, retain_graph=True)
        ref, scale = G.q_rows_bwd_ref(adj, ctx, raw, g, present, F64)
        assert float((ref - grad).abs().max()) <= 1e-12 * max(1.0, float(scale.max()))
        assert not ref[scale == 0].any()


# ---------------------------------------------------------------------------------------------------------------- segment sum
@pytest.mark.parametrize("kind", G.SEG_TARGETS)
@pytest.mark.parametrize("n", G.SEG_N)
@pytest.mark.parametrize("C_", G.SEG_C)
def test_segment_statement_is_index_add_in_list_order(C_, n, kind):
    c = G.segment_case(n, C_, kind)
    idx, order, sidx, T = c["idx"], c["order"], c["sorted_idx"], c["T"]
    assert torch.equal(torch.sort(order).values, torch.arange(n))                         # a permutation
    assert bool((sidx[1:] >= sidx[:-1]).all()) and torch.equal(idx[order], sidx)          # non-decreasing, consistent
    same = sidx[1:] == sidx[:-1]
    assert bool((order[1:][same] > order[:-1][same]).all())                               # stable: list order inside a run
    assert int(idx.min()) >= 0 and int(idx.max()) < T - 1 and bool((c["dst"].abs() > 1e-3).all())
    runs = int(sidx.unique().numel())
    assert runs == {"distinct": n, "equal": 1}.get(kind, runs) and (kind != "mixed" or n < 86 or 1 < runs < n)
    for accumulate in (0, 1):
        start = c["dst"].numpy() if accumulate else np.zeros((T, C_), dtype=np.float32)
        got, named = G.segment_rows_sum_f32(c, accumulate, start)
        want = torch.from_numpy(start).double().index_add_(0, idx, c["src"].double())
        mag = torch.zeros(T, C_, dtype=F64).index_add_(0, idx, c["src"].double().abs()) + torch.from_numpy(start).double().abs()
        assert float(((torch.from_numpy(got).double() - want).abs() / mag.clamp_min(1e-30)).max()) <= n * 2.0 ** -23
        other = np.setdiff1d(np.arange(T), named)
        assert other.size > 0 and np.array_equal(got[other].view(np.int32), start[other].view(np.int32))
        assert sorted(named.tolist()) == sorted(set(idx.tolist()))
    # list order, not another order: a run of three terms whose fp32 sum depends on it
    c3 = dict(n=3, C=1, T=2, sorted_idx=torch.zeros(3, dtype=torch.long), order=torch.tensor([0, 1, 2]),
              src=torch.tensor([[1.0], [2.0 ** -24], [2.0 ** -24]]))
    fwd, _ = G.segment_rows_sum_f32(c3, 0, np.zeros((2, 1), dtype=np.float32))
    assert float(fwd[0, 0]) == 1.0 and float(np.float32(2.0 ** -24) + np.float32(2.0 ** -24) + np.float32(1.0)) > 1.0


# ---------------------------------------------------------------------------------------------------------------- film row maps
@pytest.mark.parametrize("case", G.FILM_CASES, ids=[c[0] for c in G.FILM_CASES])
def test_film_row_maps_statement_and_its_cases(case):
    c = G.film_case(case)
    R, A, D, rows, M = c["R"], c["A"], c["D"], c["rows"], c["M"]
    vis, pos, distinct, scan, bounds = c["vis"], c["pos"], c["distinct"], c["scan"], c["bounds"]
    assert R % 2 == 0 and 2 <= R <= 16 and len(bounds) == R + 1 and bounds[0] == 0 and bounds[-1] == rows == int(M.sum())
    assert all(b1 >= b0 for b0, b1 in zip(bounds[:-1], bounds[1:]))
    assert vis.shape == (rows,) and (rows == 0 or (int(vis.min()) >= 0 and int(vis.max()) < A))
    assert distinct.shape == (D,) and torch.equal(pos[distinct], torch.arange(D)) and torch.equal(scan, torch.cumsum(M.reshape(-1).long(), 0))
    for r in range(R):
        assert torch.equal(vis[bounds[r]:bounds[r + 1]], M[r].nonzero().squeeze(1))
    per_view = M.sum(dim=1).tolist()
    if case[0] == "R2-random":
        assert rows > (R // 2) * D
    if case[0] == "R16-sparse":
        assert 0 < rows < (R // 2) * D and per_view[8] == 0 and per_view[9] == A
    if case[0] == "R16-random":
        assert per_view[4] == per_view[5] == 0 and per_view[6] == 0 and per_view[7] == A
    if case[0] == "R2-empty-vs-full":
        assert per_view == [0, A]
    if case[0] == "R2-both-empty":
        assert rows == 0 and D == 0
    row_of, src_a, src_b = G.film_row_maps_ref(c)
    # plain loops
    k = 0
    for r in range(R):
        for a in M[r].nonzero().squeeze(1).tolist():
            assert int(row_of[k]) == (r // 2) * D + int(pos[a])
            src = src_a if r % 2 == 0 else src_b
            assert int(src[int(row_of[k])]) == k
            k += 1
    assert k == rows
    named = torch.cat([src_a, src_b])
    named = named[named >= 0]
    assert named.numel() == rows and torch.equal(torch.sort(named.long()).values, torch.arange(rows))
    assert int((torch.cat([src_a, src_b]) < 0).sum()) == 2 * (R // 2) * D - rows
