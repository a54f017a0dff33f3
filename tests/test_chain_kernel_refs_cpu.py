"""Pins tests/_chain_kernel_refs.py without a GPU: the float64 statements of the chain kernels against the same networks built from
torch.nn.functional and their float64 autograd, the shared-FiLM statement against the unshared one, the integer probes' exactness
conditions for every case table of tests/test_chain_kernels_gpu.py, and the layout helper against the header's size formulas."""
import pytest
import torch
import torch.nn.functional as F

from tests import _chain_kernel_refs as R
from tests._chain_kernel_refs import COND, FEAT, HID

f64 = torch.float64
TOL = 1e-13


def _close(tag, a, b):
    scale = max(float(b.abs().max()), 1e-300) if b.numel() else 1.0
    assert a.shape == b.shape and float((a - b).abs().max() if b.numel() else 0.0) <= TOL * scale, (tag, float((a - b).abs().max()), scale)


def _act(code, v):
    return torch.tanh(v) if code == R.ACT_TANH else (torch.sigmoid(v) if code == R.ACT_SIGMOID else v)


def _leaf(t):
    return t.clone().requires_grad_(True)


def _torch_generator(n, feat, cf, row_of):
    """(tensors by the statement's names, the leaves and the intermediates whose gradients the backward statement names)."""
    w = {k: _leaf(n[k]) for k in R.GEN_W}
    hg, hb = F.linear(cf, w["Wg0"], w["bg0"]), F.linear(cf, w["Wb0"], w["bb0"])
    cg, cb = F.relu(hg), F.relu(hb)
    gamma, beta = F.linear(cg, w["Wg1"], w["bg1"]), F.linear(cb, w["Wb1"], w["bb1"])
    z1 = F.linear(feat, w["W1"], w["b1"])
    a1 = F.gelu(z1)
    h = F.linear(a1, w["W2"], w["b2"])
    x3 = (gamma if row_of is None else gamma[row_of]) * h + (beta if row_of is None else beta[row_of])
    pre = F.linear(x3, w["W3"], w["b3"])
    y = _act(n["act"], pre)
    t = {"cg": cg, "cb": cb, "gamma": gamma, "beta": beta, "a1": a1, "h": h, "x3": x3, "y": y}
    mid = {"go": pre, "gh": h, "gz1": z1, "gbeta": beta, "ggamma": gamma, "gcg": hg, "gcb": hb}
    for v in mid.values():
        v.retain_grad()
    return t, w, mid


def _torch_deform(net, feat, cond):
    W, b = [_leaf(t) for t in net["W"]], [_leaf(t) for t in net["b"]]
    x, t, mid = torch.cat([feat, cond], 1), {}, {}
    for i in range(4):
        z = F.linear(x, W[i], b[i])
        x = F.gelu(z)
        z.retain_grad()
        t[f"z{i + 1}"], t[f"a{i + 1}"], mid[f"g{i + 1}"] = z, x, z
    t["y"] = F.linear(x, W[4], b[4])
    return t, W, b, mid


@pytest.mark.parametrize("M,n,Mf", [(1, 3, None), (17, 1, None), (17, 2, None), (37, 3, None), (2, 3, 1), (17, 3, 12), (37, 3, 30)])
def test_statements_match_functional_and_autograd(M, n, Mf):
    """Every forward statement equals the network built from torch.nn.functional, every backward statement — evaluated at the
    reference's own forward values — its float64 autograd, to 1e-13 of the tensor's max."""
    c = R.cast(R.build_case("randn", M, n, Mf), f64)
    film = c["film"]
    cf, row_of = R.film_of(film, c["cond"], M)
    feats = [_leaf(c["feat"]) for _ in range(n + 1)]      # a leaf per network: its gradient is that network's part of the feature gradient
    fw = R.generators_forward_ref(c["nets"], c["feat"], c["cond"], film)
    loss, nets_t = 0.0, []
    for i, net in enumerate(c["nets"]):
        t, w, mid = _torch_generator(net, feats[i], cf, row_of)
        for k, v in t.items():
            _close(f"gen{i} {k}", fw[i][k][0], v.detach())
        loss = loss + (t["y"] * c["gys"][i]).sum()
        nets_t.append((w, mid))
    dfw = R.deform_forward_ref(c["deform"], c["feat"], c["cond"])
    dt, dW, db, dmid = _torch_deform(c["deform"], feats[n], c["cond"])
    for k, v in dt.items():
        _close(f"deform {k}", dfw[k][0], v.detach())
    (loss + (dt["y"] * c["gys"][n]).sum()).backward()
    bw = R.generators_backward_ref(c["nets"], c["feat"], cf, [R.values(o) for o in fw], [o["y"][0] for o in fw], c["gys"][:n], film)
    for i, (w, mid) in enumerate(nets_t):
        for k, v in mid.items():
            _close(f"gen{i} {k}", bw[i][k][0], v.grad)
        for k in R.GEN_W:
            _close(f"gen{i} d{k}", bw[i]["d" + k][0], w[k].grad)
        _close(f"gen{i} gfeat_part", bw[i]["gfeat_part"][0], feats[i].grad)
    dbw = R.deform_backward_ref(c["deform"], c["feat"], c["cond"], R.values(dfw), c["gys"][n], [(o["gfeat_part"][0], o["gfeat_part"][1]) for o in bw])
    for k, v in dmid.items():
        _close(f"deform {k}", dbw[k][0], v.grad)
    for i in range(5):
        _close(f"deform dW{i}", dbw[f"dW{i}"][0], dW[i].grad)
        _close(f"deform db{i}", dbw[f"db{i}"][0], db[i].grad)
    _close("gfeat_sum", dbw["gfeat_sum"][0], sum(f.grad for f in feats))
    # the single-step statements, evaluated on the chain statements' own values, give those values again
    vf, vb, vdf, vdb = [R.values(o) for o in fw], [R.values(o) for o in bw], R.values(dfw), R.values(dbw)
    steps = list(zip(R.generators_forward_steps(c["nets"], vf, film), fw)) + [(R.deform_forward_steps(c["deform"], vdf), dfw)]
    steps += list(zip(R.generators_backward_steps(c["nets"], c["feat"], c["cond"], vf, vb, film), bw))
    steps.append((R.deform_backward_steps(c["deform"], c["feat"], c["cond"], vdf, vdb, [o["gfeat_part"] for o in vb]), dbw))
    for st, full in steps:
        for k, (v, S, L) in st.items():
            _close("step " + k, v, full[k][0])
            assert L == (1 + n if k == "gfeat_sum" else 1) and bool((v.abs() <= S * (1 + 1e-12) + 1e-300).all()), k
    # every scale is non-negative and bounds its value
    for o in fw + bw + [dfw, dbw]:
        for k, (v, S, L) in o.items():
            assert L >= 1 and bool((S >= 0).all()) and bool((v.abs() <= S * (1 + 1e-12) + 1e-300).all()), k


@pytest.mark.parametrize("M,Mf", [(2, 1), (17, 12), (150, 100)])
def test_shared_film_statement_equals_unshared(M, Mf):
    """The shared statement equals the unshared one run on cond_film[row_of]; its summed d gamma / d beta equal an index_add of the
    per-view rows."""
    c = R.cast(R.build_case("randn", M, 3, Mf), f64)
    film, ro = c["film"], c["film"]["row_of"].long()
    sh = R.generators_forward_ref(c["nets"], c["feat"], c["cond"], film)
    un = R.generators_forward_ref(c["nets"], c["feat"], c["cond"], None)
    for a, b in zip(sh, un):
        for k in ("a1", "h", "x3", "y"):
            _close(k, a[k][0], b[k][0])
        for k in ("cg", "cb", "gamma", "beta"):
            _close(k, a[k][0][ro], b[k][0])
    ys = [o["y"][0] for o in un]
    bs = R.generators_backward_ref(c["nets"], c["feat"], film["cond"], [R.values(o) for o in sh], ys, c["gys"][:3], film)
    bu = R.generators_backward_ref(c["nets"], c["feat"], c["cond"], [R.values(o) for o in un], ys, c["gys"][:3], None)
    for a, b in zip(bs, bu):
        for k in ("go", "gh", "gz1", "gfeat_part", "dW1", "db1", "dW2", "db2", "dW3", "db3"):
            _close(k, a[k][0], b[k][0])
        for k in ("ggamma", "gbeta"):
            _close(k, a[k][0], torch.zeros(Mf, HID, dtype=f64).index_add_(0, ro, b[k][0]))
            _close(k + " scale", a[k][1], torch.zeros(Mf, HID, dtype=f64).index_add_(0, ro, b[k][1]))
        for k in ("dWg0", "dbg0", "dWg1", "dbg1", "dWb0", "dbb0", "dWb1", "dbb1"):      # the FiLM networks' sums over FiLM rows = over chain rows
            _close(k, a[k][0], b[k][0])


def _film_cases():
    return [(M, n, None, False) for M, n, exact in R.GEN_CASES if exact] + [(M, 3, Mf, os_) for M, Mf, os_, exact in R.SHARED_CASES if exact]


def _exact_ok(tag, o):
    for k, (v, S, L) in o.items():
        assert float(S.max()) < R.EXACT_LIMIT, (tag, k, float(S.max()))
        assert float((v - v.round()).abs().max()) <= R.EXACT_RESIDUE, (tag, k, "ref64 is not next to an integer")
        assert bool((R.exact_value(v).double() == v.round()).all()), (tag, k)


@pytest.mark.parametrize("M,n,Mf,one_sided", _film_cases(), ids=lambda v: str(v))
def test_integer_probes_are_exact(M, n, Mf, one_sided):
    """For every case the GPU test runs its exact probe on: every sum of absolute terms is below 2^24, ref64 lies within 1e-6 of an
    integer (which float32 holds) and every GELU pre-activation of the linear-regime probe is at least 8 — forward, and backward on the forward's values with the
    test-made integer y and gy.  The "one" probes likewise."""
    for kind in ("lin", "one", "one_cond"):
        c = R.cast(R.build_case(kind, M, n, Mf, one_sided), f64)
        tag = f"{kind} M{M} n{n} Mf{Mf}"
        fw = R.generators_forward_ref(c["nets"], c["feat"], c["cond"], c["film"])
        dfw = R.deform_forward_ref(c["deform"], c["feat"], c["cond"])
        acts = R.EXACT_ACTS[n] if kind == "lin" else [R.ACT_NONE] * n
        nets_b = [dict(net, act=a) for net, a in zip(c["nets"], acts)]
        cf = R.film_of(c["film"], c["cond"], M)[0]
        bw = R.generators_backward_ref(nets_b, c["feat"], cf, [R.values(o) for o in fw], c["ys"][:n], c["gys"][:n], c["film"], exact=True)
        dbw = R.deform_backward_ref(c["deform"], c["feat"], c["cond"], R.values(dfw), c["gys"][n], [o["gfeat_part"][:2] for o in bw], exact=True)
        for i, o in enumerate(fw + bw + [dfw, dbw]):
            _exact_ok(f"{tag} #{i}", o)
        if kind == "lin":
            for net in c["nets"]:
                assert float(R.linear_ref(c["feat"], net["W1"], net["b1"])[0].min()) >= R.GELU_LINEAR_FROM, tag
            assert min(float(dfw[f"z{i}"][0].min()) for i in (1, 2, 3, 4)) >= R.GELU_LINEAR_FROM, tag
            for net in c["nets"]:      # the ReLU really masks, and really passes
                for k in ("bg0", "bb0"):
                    assert 0.2 < float((net[k] <= -20).double().mean()) < 0.5, (tag, k)
            assert all(float((o["cg"][0] == 0).double().mean()) > 0.2 and float((o["cg"][0] > 0).double().mean()) > 0.2 for o in fw), tag
            assert set(R.probe_rows(M)) >= {0, M - 1} | ({15, 16} if M > 16 else set())
            for i in range(n + 1):
                assert bool((c["gys"][i][[r for r in range(M) if r not in set(R.probe_rows(M))]] == 0).all()), tag


def test_quant_statements_match_functional_and_autograd():
    """The quant_step statements against torch.nn.functional and float64 autograd, a NULL dq counting as zeros."""
    nets, (X, dq) = R.cast(R.make_quant("randn", 1), f64), R.cast(R.make_quant_rows("randn", 37, 2), f64)
    dq[1] = None
    Xl = _leaf(X)
    fw = R.quant_nets_forward_ref(nets, X)
    loss, zs = 0.0, []
    for i, n in enumerate(nets):
        z = F.linear(Xl, n["W1"], n["b1"])
        z.retain_grad()
        a = F.gelu(z)
        q = F.linear(a, n["W2"], n["b2"]).view(-1)
        for k, v in (("z", z), ("a", a), ("q", q)):
            _close(k, fw[i][k][0], v.detach())
        if dq[i] is not None:
            loss = loss + (q * dq[i]).sum()
        zs.append(z)
    loss.backward()
    bw, dX = R.quant_nets_backward_ref(nets, [o["z"][0] for o in fw], dq)
    for i in range(3):
        _close("dz", bw[i]["dz"][0], zs[i].grad if zs[i].grad is not None else torch.zeros_like(zs[i]))
    _close("dX", dX[0], Xl.grad)
    st, st_dX = R.quant_nets_steps(nets, [R.values(o) for o in fw], [R.values(o) for o in bw])
    for i in range(3):
        _close("step a", st[i]["a"][0], fw[i]["a"][0])
        _close("step q", st[i]["q"][0], fw[i]["q"][0])
    _close("step dX", st_dX[0], dX[0])


@pytest.mark.parametrize("M", R.QUANT_M)
def test_quant_integer_probes_are_exact(M):
    """The exactness conditions of the quant_step probes at every row count the GPU test uses."""
    for kind in ("lin", "one"):
        nets, (X, dq) = R.cast(R.make_quant(kind, 50 + M), f64), R.cast(R.make_quant_rows(kind, M, 60 + M), f64)
        fw = R.quant_nets_forward_ref(nets, X)
        bw, dX = R.quant_nets_backward_ref(nets, [o["z"][0] for o in fw], dq, exact=True)
        for i, o in enumerate(fw + bw + [{"dX": dX}]):
            _exact_ok(f"quant {kind} M{M} #{i}", o)
        if kind == "lin":
            assert min(float(o["z"][0].min()) for o in fw) >= R.GELU_LINEAR_FROM


def test_film_maps_name_every_chain_row_once():
    """Every map the GPU test uses satisfies the header's precondition; together they hold FiLM rows with both sides, only a, only b
    and neither, orders that do not increase, and Mf = 1."""
    seen = [0, 0, 0, 0]
    for M, Mf, one_sided, _ in R.SHARED_CASES + [(M, Mf, False, True) for M, Mf in R.INFERENCE_SHARED.items()]:
        row_of, src_a, src_b = R.film_map(M, Mf, 3, one_sided)
        named = torch.cat([src_a[src_a >= 0], src_b[src_b >= 0]]).long()
        assert sorted(named.tolist()) == list(range(M)), (M, Mf)
        for src in (src_a, src_b):
            q = (src >= 0).nonzero().view(-1)
            assert bool((row_of[src[q].long()] == q.int()).all()), (M, Mf)
        seen = [a + b for a, b in zip(seen, R.map_kinds(src_a, src_b))]
        if Mf > 2:
            a = src_a[src_a >= 0]
            assert bool((a[1:] < a[:-1]).any()), (M, Mf, "src_a increases")
        if one_sided:
            assert R.map_kinds(src_a, src_b)[0] == 0
    assert min(seen) > 0 and any(Mf == 1 for _, Mf, _, _ in R.SHARED_CASES)


def test_layouts_stay_within_the_size_formulas():
    """The region ends of the layout helper stay within 3 HID M + (2 COND + 2 HID) Mf + 64 and the header's other formulas, every
    region starts on a multiple of 4 floats, and no two regions overlap."""
    for M, Mf in [(1, 1), (2, 1), (15, 15), (17, 12), (17, 17), (129, 129), (150, 100), (4097, 2500), (11003, 11003), (32785, 32785)]:
        lays = [(R.gen_saved_layout(M, Mf), R.gen_saved_floats(M, Mf)), (R.gen_saved_layout(M, Mf, True), R.gen_inference_floats(M, Mf)),
                (R.deform_saved_layout(M), R.deform_saved_floats(M)), (R.deform_saved_layout(M, True), R.deform_inference_floats(M)),
                (R.deform_scratch_layout(M), R.deform_scratch_floats_min(M))]
        lays += [(R.gen_scratch_layout(M, Mf, out), R.gen_scratch_floats_min(M, Mf, out)) for out in R.GEN_OUTS]
        for (lay, end), size in lays:
            assert end <= size, (M, Mf, end, size)
            at = 0
            for name, (off, rows, cols) in lay.items():
                assert off % 4 == 0 and off >= at, (M, Mf, name)
                at = off + rows * cols
            assert at <= end
    lay = R.gen_saved_layout(17, 12)[0]
    assert lay["gamma"][:2] == (0, 12) and lay["cg"] == (2 * 1200, 12, COND) and lay["a1"][0] == 2400 + 2 * 792 and lay["x3"] == (2400 + 1584 + 3400, 17, HID)
    assert R.deform_scratch_layout(3)[0]["stage_c"] == (1200 + HID * FEAT, HID, COND)
