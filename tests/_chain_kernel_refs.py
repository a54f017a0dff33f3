"""Plain tensor statements of the whole-network chain kernels (csrc/mlp_chain.hip), one per C entry, written from include/gsvc_hip.h:
gsvc_generate_all_forward / _backward (the generators and the deformation network) and gsvc_quant_step_nets_forward / _backward.
Called with float64 tensors they are the references of tests/test_chain_kernels_gpu.py; called with float32 tensors they are "the
fp32 tensor statement" those tests calibrate against.  tests/test_chain_kernel_refs_cpu.py pins them, the layout helper, the input
generators and the case tables below without a GPU.  Nothing here imports the package under test.

Every statement returns, for every tensor its entry writes, (value, scale, L):
  * scale: the sum of absolute terms CARRIED through the chain, formed from inputs and reference values only.  S(input) = |input|;
    through a product S |W|^T + |b|; through ReLU or a mask unchanged; through GELU, tanh or sigmoid max(1, S); through FiLM
    S_gamma S_h + S_beta; for g GELU'(z) S_g max(1, S_z); for g act'(y) S_g max(1, |y|)^2; for a weight gradient S_G^T S_X; for a
    sum the sum of the parts' scales.
  * L: the number of matrix products between the entry's inputs and the tensor, its own included, at least 1 (the longest path
    where two meet).  The float64 rule of the GPU test allows one rounding per product: e <= 4 e32 + 4 L eps32.
"""
import torch

from tests._linear_kernel_refs import EPS32, PRINT, err, gelu, gelu_grad, ints, linear_ref, normal, wgrad_ref  # noqa: F401

FEAT, COND, HID = 50, 66, 100            # the instantiated widths
GEN_OUTS = (10, 30, 70)
DEF_OUT = 30
Q_IN, Q_HID = 192, 50
ACT_NONE, ACT_TANH, ACT_SIGMOID = 0, 1, 2
EXACT_LIMIT = float(2 ** 24)
GELU_LINEAR_FROM = 8.0                   # z >= 8: the kernels' GELU is the identity and its derivative 1 in fp32 (q = 0.5 p e < 2^-25)

GEN_W = ("W1", "b1", "W2", "b2", "W3", "b3", "Wg0", "bg0", "Wg1", "bg1", "Wb0", "bb0", "Wb1", "bb1")      # order of gsvc_generator_net
# (out_dim, out_act) of the generators of a call with n networks: all three widths and all three activations with n = 3
GEN_SETS = {1: ((70, ACT_TANH),), 2: ((30, ACT_SIGMOID), (10, ACT_NONE)), 3: ((10, ACT_TANH), (30, ACT_SIGMOID), (70, ACT_NONE))}


# exact_note.  The backward statements take exact=True for the linear-regime integer probe.  There every GELU pre-activation is >= 8,
# so GELU'(z) is exactly 1 and g GELU'(z) has the single term g, and y is a small integer, so act'(y) is an exact integer and
# gy act'(y) has the single term |gy act'(y)|.  The factors max(1, S_z) and max(1, |y|)^2 of the float64 rule's scale stand for the
# ERROR of a transcendental factor, not for terms of a sum: carried through four layers they exceed 2^24 by construction (the
# deformation network's pre-activations are at least 8, 24, 56 and 120) although no fp32 sum of the probe comes near it.  With
# exact=True the two factors are 1 and |act'(y)|: the scale is then the true sum of absolute terms of the fp32 evaluation, which is
# what has to stay below 2^24 for the result to be exact in any summation order.

#
# The float64 statement itself is not exactly integer there: GELU'(8) = 1 + 4e-14 and GELU(8) = 8 (1 - 6e-16) in float64, and where
# integer terms cancel such a residue is all that is left.  The exact expectation is therefore exact_value(ref64), the nearest
# integer; the CPU test shows that ref64 lies within EXACT_RESIDUE of it, so it is the integer the linear-regime result is.
EXACT_RESIDUE = 1e-6


def exact_value(ref64):
    """The fp32 tensor an exact probe must give: the integer next to the float64 statement's value."""
    return ref64.round().to(torch.float32)


# ------------------------------------------------------------------------------------------------------------ pieces
def _carry(S, W, b=None, w_in_out=False):
    """The scale through a product: S |W|^T + |b| (S |W| for w_in_out)."""
    return linear_ref(S, W.abs(), None if b is None else b.abs(), w_in_out)[0]


def _one(S):
    return torch.clamp_min(S, 1.0)


def _act(code, v):
    if code == ACT_TANH:
        return torch.tanh(v)
    if code == ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-v))
    assert code == ACT_NONE
    return v


def _act_grad_from_y(code, y):
    """act'(pre-activation) written in the output y: 1 - y^2 (tanh), (1 - y) y (sigmoid)."""
    if code == ACT_TANH:
        return 1.0 - y * y
    if code == ACT_SIGMOID:
        return (1.0 - y) * y
    return torch.ones_like(y)


def _wgrad(out, name, bname, G, S_G, X, S_X, L):
    dW, db = wgrad_ref(G, X)[:2]
    out[name], out[bname] = (dW, S_G.t() @ S_X, L), (db, S_G.sum(0), L)


def film_of(film, cond, M):
    """(FiLM rows' condition, row_of or None): film = None (one FiLM row per chain row) or a dict cond / row_of / src_a / src_b."""
    if film is None:
        return cond, None
    return film["cond"], film["row_of"].long()


# ------------------------------------------------------------------------------------------------------------ generators
def generators_forward_ref(nets, feat, cond, film=None):
    """Per network {cg, cb, gamma, beta (one row per FiLM row), a1, h, x3, y (one row per chain row)}: (value, scale, L).
    gamma = Wg1 relu(Wg0 c + bg0) + bg1, beta likewise; y = act(W3 (gamma[row_of] * (W2 gelu(W1 f + b1) + b2) + beta[row_of]) + b3)."""
    cf, row_of = film_of(film, cond, feat.shape[0])
    res = []
    for n in nets:
        o = {}
        v, S = linear_ref(cf, n["Wg0"], n["bg0"])
        cg, S_cg = torch.clamp_min(v, 0), S
        v, S = linear_ref(cf, n["Wb0"], n["bb0"])
        cb, S_cb = torch.clamp_min(v, 0), S
        gamma, S_gamma = linear_ref(cg, n["Wg1"], n["bg1"])[0], _carry(S_cg, n["Wg1"], n["bg1"])
        beta, S_beta = linear_ref(cb, n["Wb1"], n["bb1"])[0], _carry(S_cb, n["Wb1"], n["bb1"])
        o["cg"], o["cb"], o["gamma"], o["beta"] = (cg, S_cg, 1), (cb, S_cb, 1), (gamma, S_gamma, 2), (beta, S_beta, 2)
        z1, S_z1 = linear_ref(feat, n["W1"], n["b1"])
        a1, S_a1 = gelu(z1), _one(S_z1)
        h, S_h = linear_ref(a1, n["W2"], n["b2"])[0], _carry(S_a1, n["W2"], n["b2"])
        g_r, b_r, Sg_r, Sb_r = (gamma, beta, S_gamma, S_beta) if row_of is None else (gamma[row_of], beta[row_of], S_gamma[row_of], S_beta[row_of])
        x3, S_x3 = g_r * h + b_r, Sg_r * S_h + Sb_r
        pre, S_pre = linear_ref(x3, n["W3"], n["b3"])[0], _carry(S_x3, n["W3"], n["b3"])
        y, S_y = _act(n["act"], pre), (S_pre if n["act"] == ACT_NONE else _one(S_pre))
        o["a1"], o["h"], o["x3"], o["y"] = (a1, S_a1, 1), (h, S_h, 2), (x3, S_x3, 2), (y, S_y, 3)
        res.append(o)
    return res


def generators_backward_ref(nets, feat, cond, saved, y, gy, film=None, exact=False):
    """Per network, from what the backward is handed (saved[i]: cg, cb, gamma, a1, h, x3; y[i]; gy[i]; feat; the FiLM rows' condition):
      per chain row  go = gy act'(y), gh = (go W3) gamma[row_of], gz1 = (gh W2) gelu'(W1 f + b1), gfeat_part = gz1 W1
      per FiLM row   gbeta = sum of go W3 over the row's chain rows, ggamma = sum of (go W3) h, gcg = (ggamma Wg1) [cg > 0], gcb likewise
      and the seven weight / bias gradients dW = G^T X, db = column sums of G.
    exact: the scales of the linear-regime integer probe (see exact_note)."""
    cf, row_of = film_of(film, cond, feat.shape[0])
    res = []
    for n, sv, yy, g in zip(nets, saved, y, gy):
        o = {}
        go = g * _act_grad_from_y(n["act"], yy)
        S_go = go.abs() if (exact or n["act"] == ACT_NONE) else g.abs() * _one(yy.abs()) ** 2
        gx3, S_gx3 = go @ n["W3"], S_go @ n["W3"].abs()
        gam_r = sv["gamma"] if row_of is None else sv["gamma"][row_of]
        dg, S_dg = gx3 * sv["h"], S_gx3 * sv["h"].abs()
        gh, S_gh = gx3 * gam_r, S_gx3 * gam_r.abs()
        z1, S_z1 = linear_ref(feat, n["W1"], n["b1"])
        gz1, S_gz1 = (gh @ n["W2"]) * gelu_grad(z1), (S_gh @ n["W2"].abs()) * (1.0 if exact else _one(S_z1))
        gfeat, S_gfeat = gz1 @ n["W1"], S_gz1 @ n["W1"].abs()
        if row_of is None:
            gbeta, S_gbeta, ggamma, S_ggamma = gx3, S_gx3, dg, S_dg
        else:
            Mf = cf.shape[0]
            acc = lambda t: torch.zeros(Mf, HID, dtype=t.dtype, device=t.device).index_add_(0, row_of, t)  # noqa: E731
            gbeta, S_gbeta, ggamma, S_ggamma = acc(gx3), acc(S_gx3), acc(dg), acc(S_dg)
        zero = torch.zeros((), dtype=feat.dtype, device=feat.device)
        gcg, S_gcg = torch.where(sv["cg"] > 0, ggamma @ n["Wg1"], zero), S_ggamma @ n["Wg1"].abs()
        gcb, S_gcb = torch.where(sv["cb"] > 0, gbeta @ n["Wb1"], zero), S_gbeta @ n["Wb1"].abs()
        o["go"], o["gh"], o["gz1"], o["gfeat_part"] = (go, S_go, 1), (gh, S_gh, 1), (gz1, S_gz1, 2), (gfeat, S_gfeat, 3)
        o["gbeta"], o["ggamma"], o["gcg"], o["gcb"] = (gbeta, S_gbeta, 1), (ggamma, S_ggamma, 1), (gcg, S_gcg, 2), (gcb, S_gcb, 2)
        _wgrad(o, "dW1", "db1", gz1, S_gz1, feat, feat.abs(), 3)
        _wgrad(o, "dW2", "db2", gh, S_gh, sv["a1"], sv["a1"].abs(), 2)
        _wgrad(o, "dW3", "db3", go, S_go, sv["x3"], sv["x3"].abs(), 1)
        _wgrad(o, "dWg0", "dbg0", gcg, S_gcg, cf, cf.abs(), 3)
        _wgrad(o, "dWg1", "dbg1", ggamma, S_ggamma, sv["cg"], sv["cg"].abs(), 2)
        _wgrad(o, "dWb0", "dbb0", gcb, S_gcb, cf, cf.abs(), 3)
        _wgrad(o, "dWb1", "dbb1", gbeta, S_gbeta, sv["cb"], sv["cb"].abs(), 2)
        res.append(o)
    return res


# ------------------------------------------------------------------------------------------------------------ mlp_deform
def deform_forward_ref(net, feat, cond):
    """{z1, a1, .., z4, a4, y}: five Linear layers with GELU between on [feat | cond]."""
    o = {}
    x, S = torch.cat([feat, cond], 1), torch.cat([feat, cond], 1).abs()
    for i in range(4):
        z, S_z = linear_ref(x, net["W"][i], net["b"][i])[0], _carry(S, net["W"][i], net["b"][i])
        x, S = gelu(z), _one(S_z)
        o[f"z{i + 1}"], o[f"a{i + 1}"] = (z, S_z, i + 1), (x, S, i + 1)
    o["y"] = (linear_ref(x, net["W"][4], net["b"][4])[0], _carry(S, net["W"][4], net["b"][4]), 5)
    return o


def deform_backward_ref(net, feat, cond, saved, gy, parts=(), exact=False):
    """{g4, g3, g2, g1, gfeat_sum, dW0 .. dW4, db0 .. db4} from saved (z1, a1, .., z4, a4) and gy: g4 = (gy W5) gelu'(z4), g_i =
    (g_{i+1} W_{i+1}) gelu'(z_i); gfeat_sum = g1 W1[:, :FEAT] + the generators' parts ((value, scale) pairs); dW0 = [g1^T feat | g1^T cond]."""
    o = {}
    g, S = gy, gy.abs()
    G = {5: (g, S)}
    for i in (4, 3, 2, 1):
        W = net["W"][i]
        g, S = (g @ W) * gelu_grad(saved[f"z{i}"]), (S @ W.abs()) * (1.0 if exact else _one(saved[f"z{i}"].abs()))
        G[i] = (g, S)
        o[f"g{i}"] = (g, S, 5 - i)
    W1f = net["W"][0][:, :FEAT]
    gf, S_gf = G[1][0] @ W1f, G[1][1] @ W1f.abs()
    for v, s in parts:
        gf, S_gf = gf + v, S_gf + s
    o["gfeat_sum"] = (gf, S_gf, 5)
    x = torch.cat([feat, cond], 1)
    _wgrad(o, "dW0", "db0", G[1][0], G[1][1], x, x.abs(), 5)
    for i in (1, 2, 3, 4):
        a = saved[f"a{i}"]
        _wgrad(o, f"dW{i}", f"db{i}", G[i + 1][0], G[i + 1][1], a, a.abs(), 5 - i)
    return o


# ------------------------------------------------------------------------------------------------------------ quant_step nets
def quant_nets_forward_ref(nets, X):
    """Per network {z = X W1^T + b1, a = gelu(z), q = a W2^T + b2 [M]}."""
    res = []
    for n in nets:
        z, S_z = linear_ref(X, n["W1"], n["b1"])
        a, S_a = gelu(z), _one(S_z)
        q, S_q = linear_ref(a, n["W2"], n["b2"])[0], _carry(S_a, n["W2"], n["b2"])
        res.append({"z": (z, S_z, 1), "a": (a, S_a, 2), "q": (q.reshape(-1), S_q.reshape(-1), 2)})
    return res


def quant_nets_backward_ref(nets, z, dq, exact=False):
    """({dz_i = dq_i W2_i gelu'(z_i)} per network, dX = sum_i dz_i W1_i); dq[i] None counts as zeros."""
    res, dX, S_dX = [], None, None
    for n, zz, d in zip(nets, z, dq):
        d = torch.zeros(zz.shape[0], dtype=zz.dtype, device=zz.device) if d is None else d
        dz = d[:, None] * n["W2"].reshape(1, -1) * gelu_grad(zz)
        S_dz = d.abs()[:, None] * n["W2"].abs().reshape(1, -1) * (1.0 if exact else _one(zz.abs()))
        res.append({"dz": (dz, S_dz, 2)})
        v, s = dz @ n["W1"], S_dz @ n["W1"].abs()
        dX, S_dX = (v, s) if dX is None else (dX + v, S_dX + s)
    return res, (dX, S_dX, 2)


# ------------------------------------------------------------------------------------------------------------ single steps
# The carried scale grows with the depth of the chain (the generators' S_y is about 10^4 |y|), so the chain-long rule says little about
# the last steps of a chain.  Every tensor of a chain crosses HBM, though: each stored tensor can also be held against the statement
# of ITS OWN STEP, evaluated on the stored tensors that step read — one product, L = 1, the scale the plain sum of absolute terms of
# that product.  `got` holds the kernel's tensors (cast to the dtype of the run).  Tensors whose step reads the entry's inputs alone
# (cg, cb, a1 of a generator, z1 of the deformation network, go, g4, dW3 of a generator, dW4) are L = 1 in the chain statements already.
def generators_forward_steps(nets, got, film=None):
    """Per network {gamma, beta, h, x3, y} from the stored cg, cb, a1, (gamma, beta, h), x3."""
    res = []
    for n, g in zip(nets, got):
        o = {}
        o["gamma"] = linear_ref(g["cg"], n["Wg1"], n["bg1"]) + (1,)
        o["beta"] = linear_ref(g["cb"], n["Wb1"], n["bb1"]) + (1,)
        o["h"] = linear_ref(g["a1"], n["W2"], n["b2"]) + (1,)
        gam, bet = (g["gamma"], g["beta"]) if film is None else (g["gamma"][film["row_of"].long()], g["beta"][film["row_of"].long()])
        o["x3"] = (gam * g["h"] + bet, gam.abs() * g["h"].abs() + bet.abs(), 1)
        pre, A = linear_ref(g["x3"], n["W3"], n["b3"])
        o["y"] = (_act(n["act"], pre), A if n["act"] == ACT_NONE else _one(A), 1)
        res.append(o)
    return res


def deform_forward_steps(net, got):
    """{a1 .. a4, z2 .. z4, y} from the stored z_i (a_i = gelu(z_i)) and a_i (z_{i+1} = W a_i + b)."""
    o = {}
    for i in (1, 2, 3, 4):
        o[f"a{i}"] = (gelu(got[f"z{i}"]), _one(got[f"z{i}"].abs()), 1)
        o[f"z{i + 1}" if i < 4 else "y"] = linear_ref(got[f"a{i}"], net["W"][i], net["b"][i]) + (1,)
    return o


def generators_backward_steps(nets, feat, cond, saved, got, film=None):
    """Per network {gz1, gfeat_part, gcg, gcb, the weight gradients but dW3 / db3} from the stored gh, gz1, ggamma, gbeta, gcg, gcb; with one
    FiLM row per chain row also {gbeta, ggamma, gh} from the stored go and gbeta (with shared rows the per-view gbeta is never stored)."""
    cf = cond if film is None else film["cond"]
    res = []
    for n, sv, g in zip(nets, saved, got):
        o = {}
        z1, S_z1 = linear_ref(feat, n["W1"], n["b1"])
        o["gz1"] = ((g["gh"] @ n["W2"]) * gelu_grad(z1), (g["gh"].abs() @ n["W2"].abs()) * _one(S_z1), 1)
        o["gfeat_part"] = (g["gz1"] @ n["W1"], g["gz1"].abs() @ n["W1"].abs(), 1)
        zero = torch.zeros((), dtype=feat.dtype, device=feat.device)
        o["gcg"] = (torch.where(sv["cg"] > 0, g["ggamma"] @ n["Wg1"], zero), g["ggamma"].abs() @ n["Wg1"].abs(), 1)
        o["gcb"] = (torch.where(sv["cb"] > 0, g["gbeta"] @ n["Wb1"], zero), g["gbeta"].abs() @ n["Wb1"].abs(), 1)
        if film is None:
            o["gbeta"] = (g["go"] @ n["W3"], g["go"].abs() @ n["W3"].abs(), 1)
            o["ggamma"] = (g["gbeta"] * sv["h"], g["gbeta"].abs() * sv["h"].abs(), 1)
            o["gh"] = (g["gbeta"] * sv["gamma"], g["gbeta"].abs() * sv["gamma"].abs(), 1)
        for w, G, X in (("W1", g["gz1"], feat), ("W2", g["gh"], sv["a1"]), ("Wg0", g["gcg"], cf), ("Wg1", g["ggamma"], sv["cg"]),
                        ("Wb0", g["gcb"], cf), ("Wb1", g["gbeta"], sv["cb"])):
            dW, db, SW, Sb = wgrad_ref(G, X)
            o["d" + w], o["db" + w[1:]] = (dW, SW, 1), (db, Sb, 1)
        res.append(o)
    return res


def deform_backward_steps(net, feat, cond, saved, got, parts):
    """{g3, g2, g1, gfeat_sum, dW0 .. dW3, db0 .. db3} from the stored g4 .. g1 and the stored generators' parts (L = 1, but gfeat_sum:
    1 + the number of parts)."""
    o = {}
    for i in (3, 2, 1):
        g, W, z = got[f"g{i + 1}"], net["W"][i], saved[f"z{i}"]
        o[f"g{i}"] = ((g @ W) * gelu_grad(z), (g.abs() @ W.abs()) * _one(z.abs()), 1)
    W1f = net["W"][0][:, :FEAT]
    v, S = got["g1"] @ W1f, got["g1"].abs() @ W1f.abs()
    for t in parts:
        v, S = v + t, S + t.abs()
    # the kernel adds the parts first and accumulates its product on top: every part added is one more rounding at the magnitude of
    # the whole sum, like a product of a chain (L counts roundings at the scale's magnitude)
    o["gfeat_sum"] = (v, S, 1 + len(parts))
    x = torch.cat([feat, cond], 1)
    for i in range(4):
        dW, db, SW, Sb = wgrad_ref(got[f"g{i + 1}"], x if i == 0 else saved[f"a{i}"])
        o[f"dW{i}"], o[f"db{i}"] = (dW, SW, 1), (db, Sb, 1)
    return o


def quant_nets_steps(nets, got_fw, got_bw):
    """({a, q} per network from the stored z and a, dX from the stored dz)."""
    res, dX, S = [], None, None
    for n, g, b in zip(nets, got_fw, got_bw):
        q, A = linear_ref(g["a"], n["W2"], n["b2"])
        res.append({"a": (gelu(g["z"]), _one(g["z"].abs()), 1), "q": (q.reshape(-1), A.reshape(-1), 1)})
        v, s = b["dz"] @ n["W1"], b["dz"].abs() @ n["W1"].abs()
        dX, S = (v, s) if dX is None else (dX + v, S + s)
    return res, (dX, S, 1)


# ------------------------------------------------------------------------------------------------------------ layouts
# These mirror GenSaved, GenScratch, DeformSaved and DeformScratch of csrc/mlp_chain.hip and change with them: every region of the
# generators' buffers is rounded up to 4 floats (take()); the deformation network's regions follow each other directly and its two
# staging matrices and the weight gradients' workspace start 16-byte aligned (align16: the same rounding for an aligned base).
def _r4(n):
    return (n + 3) // 4 * 4


def _lay(regions):
    off, out = 0, {}
    for name, rows, cols in regions:
        out[name] = (off, rows, cols)
        off = _r4(off + rows * cols)
    return out, off


def gen_saved_layout(M, Mf, inference=False):
    """({name: (offset, rows, cols)}, end of the last region)."""
    reg = [("gamma", Mf, HID), ("beta", Mf, HID)]
    if not inference:
        reg += [("cg", Mf, COND), ("cb", Mf, COND), ("a1", M, HID), ("h", M, HID), ("x3", M, HID)]
    return _lay(reg)


def gen_scratch_layout(M, Mf, out):
    """The end is where the weight gradients' partial sums begin."""
    return _lay([("go", M, out), ("gh", M, HID), ("gz1", M, HID), ("gbeta", Mf, HID), ("ggamma", Mf, HID), ("gcg", Mf, COND), ("gcb", Mf, COND)])


def deform_saved_layout(M, inference=False):
    if inference:
        return _lay([("a2", M, HID)])
    return _lay([(k, M, HID) for k in ("z1", "a1", "z2", "a2", "z3", "a3", "z4", "a4")])


def deform_scratch_layout(M):
    return _lay([("g1", M, HID), ("g2", M, HID), ("g3", M, HID), ("g4", M, HID), ("stage_f", HID, FEAT), ("stage_c", HID, COND)])


# the size formulas of include/gsvc_hip.h (the scratch sizes without the weight gradients' workspace, which follows the regions)
def gen_saved_floats(M, Mf):
    return 3 * HID * M + (2 * COND + 2 * HID) * Mf + 64


def gen_inference_floats(M, Mf):
    return 2 * HID * Mf + 64


def gen_scratch_floats_min(M, Mf, out):
    return (out + 2 * HID) * M + (2 * COND + 2 * HID) * Mf + 96


def deform_saved_floats(M):
    return 8 * HID * M


def deform_inference_floats(M):
    return HID * M


def deform_scratch_floats_min(M):
    return 4 * HID * M + 2 * HID * (FEAT + COND) + 64


def views(buf, layout):
    """{name: [rows, cols] view} of a flat buffer."""
    return {k: buf[o:o + r * c].view(r, c) for k, (o, r, c) in layout.items()}


# ------------------------------------------------------------------------------------------------------------ inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _sparse01(N, K, seed):
    """{0, 1} weights, two non-zeros per row at random columns, and W[N - 1][K - 1] = 1 always."""
    g = _gen(seed)
    W = torch.zeros(N, K)
    cols = torch.stack([torch.randperm(K, generator=g)[:2] for _ in range(N)])
    W.scatter_(1, cols, 1.0)
    W[N - 1, K - 1] = 1.0
    return W


def _rint(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).to(torch.float32)


def make_generators(kind, n_nets, seed, acts=None):
    """n_nets generator networks (dicts of fp32 CPU tensors + out, act).
    "randn": normal weights scaled by K^-0.5, biases by 0.5 (gamma / beta come out O(1)), the activations of GEN_SETS;
    "lin": the linear-regime probe: {0, 1} weights with two non-zeros per row, b1 (in front of the GELU) integers in [8, 11], a third of
           bg0 / bb0 at -20 (the ReLU masks: the condition sums stay below 10) and the rest in [8, 11], the other biases in [-3, 3];
    "one", "one_cond": zeros but one path to the last output: W1[99][49], W2[99][99], W3[out - 1][99], Wg0 / Wb0[65][65], Wg1 / Wb1[99][65].
    acts: the output activations (default: GEN_SETS for "randn", none for the integer kinds)."""
    nets = []
    for i, (out, act) in enumerate(GEN_SETS[n_nets]):
        s = seed + 100 * i
        dims = {"W1": (HID, FEAT), "W2": (HID, HID), "W3": (out, HID), "Wg0": (COND, COND), "Wg1": (HID, COND), "Wb0": (COND, COND), "Wb1": (HID, COND)}
        n = {"out": out, "act": (act if kind == "randn" else ACT_NONE) if acts is None else acts[i]}
        for j, (w, (N, K)) in enumerate(dims.items()):
            b = "b" + w[1:]
            if kind == "randn":
                n[w], n[b] = normal((N, K), s + 2 * j, K ** -0.5), normal((N,), s + 2 * j + 1, 0.5)
            elif kind == "lin":
                n[w] = _sparse01(N, K, s + 2 * j)
                if w == "W1":
                    n[b] = _rint((N,), 8, 11, s + 2 * j + 1)
                elif w in ("Wg0", "Wb0"):
                    n[b] = _rint((N,), 8, 11, s + 2 * j + 1)
                    n[b][(1 if w == "Wg0" else 2)::3] = -20.0
                else:
                    n[b] = _rint((N,), -3, 3, s + 2 * j + 1)
            else:
                assert kind in ("one", "one_cond")
                n[w], n[b] = torch.zeros(N, K), torch.zeros(N)
                n[w][N - 1, K - 1] = 1.0
        nets.append(n)
    return nets


def make_deform(kind, seed):
    """The deformation network {W: [5], b: [5]}; the kinds of make_generators ("one": W1[99][49] in the feature half, "one_cond":
    W1[99][115] in the condition half)."""
    dims = [(HID, FEAT + COND), (HID, HID), (HID, HID), (HID, HID), (DEF_OUT, HID)]
    W, b = [], []
    for i, (N, K) in enumerate(dims):
        if kind == "randn":
            W.append(normal((N, K), seed + 2 * i, K ** -0.5))
            b.append(normal((N,), seed + 2 * i + 1, 0.5))
        elif kind == "lin":
            W.append(_sparse01(N, K, seed + 2 * i))
            b.append(_rint((N,), 8, 11, seed + 2 * i + 1) if i < 4 else _rint((N,), -3, 3, seed + 2 * i + 1))
        else:
            w = torch.zeros(N, K)
            w[N - 1, (FEAT - 1 if kind == "one" else K - 1) if i == 0 else K - 1] = 1.0
            W.append(w)
            b.append(torch.zeros(N))
    return {"W": W, "b": b}


def make_rows(kind, M, Mf, seed):
    """(feat [M, FEAT], the FiLM rows' condition [Mf, COND]).  "randn"; "lin": integers in [0, 3]; "one": feat[M - 1][49] = 8 (GELU(8) = 8
    in fp32) and cond[Mf - 1][65] = 2 alone; "one_cond": cond[Mf - 1][65] = 8 alone."""
    if kind == "randn":
        return normal((M, FEAT), seed), normal((Mf, COND), seed + 1)
    if kind == "lin":
        return _rint((M, FEAT), 0, 3, seed), _rint((Mf, COND), 0, 3, seed + 1)
    feat, cond = torch.zeros(M, FEAT), torch.zeros(Mf, COND)
    if kind == "one":
        feat[M - 1, FEAT - 1] = 8.0
        cond[Mf - 1, COND - 1] = 2.0
    else:
        assert kind == "one_cond"
        cond[Mf - 1, COND - 1] = 8.0
    return feat, cond


def probe_rows(M):
    """The rows that carry a gradient in the exact backward probe: 0, 15, 16, M - 1 and one in every 509."""
    return sorted({r for r in (0, 15, 16, M - 1) if 0 <= r < M} | set(range(7, M, 509)))


def backward_probe(kind, M, outs, seed):
    """(y, gy) per output width.  "randn": gy normal, y None (the forward's own y is used); "lin": y integers in [-2, 2] (1 - y^2 and
    (1 - y) y are then exact), gy integers in [-2, 2] on probe_rows(M) and zero elsewhere; "one" / "one_cond": y zeros, gy[M - 1][out - 1] =
    1 alone."""
    ys, gys = [], []
    for i, out in enumerate(outs):
        if kind == "randn":
            ys.append(None)
            gys.append(normal((M, out), seed + 10 * i))
        elif kind == "lin":
            ys.append(ints((M, out), 2, seed + 10 * i))
            g = torch.zeros(M, out)
            rows = torch.tensor(probe_rows(M))
            g[rows] = ints((len(rows), out), 2, seed + 10 * i + 1)
            gys.append(g)
        else:
            ys.append(torch.zeros(M, out))
            g = torch.zeros(M, out)
            g[M - 1, out - 1] = 1.0
            gys.append(g)
    return ys, gys


def make_quant(kind, seed):
    """Three quant_step networks {W1 [50, 192], b1, W2 [1, 50], b2 [1]}.  "lin": W1 in {0, 1} (two per row), b1 in [8, 11], W2 and b2
    integers in [-2, 2]; "one": W1[49][191] = 1 and W2[49] = 1 alone."""
    nets = []
    for i in range(3):
        s = seed + 10 * i
        if kind == "randn":
            nets.append({"W1": normal((Q_HID, Q_IN), s, Q_IN ** -0.5), "b1": normal((Q_HID,), s + 1, 0.5),
                         "W2": normal((1, Q_HID), s + 2, Q_HID ** -0.5), "b2": normal((1,), s + 3, 0.5)})
        elif kind == "lin":
            nets.append({"W1": _sparse01(Q_HID, Q_IN, s), "b1": _rint((Q_HID,), 8, 11, s + 1), "W2": ints((1, Q_HID), 2, s + 2),
                         "b2": ints((1,), 2, s + 3)})
        else:
            n = {"W1": torch.zeros(Q_HID, Q_IN), "b1": torch.zeros(Q_HID), "W2": torch.zeros(1, Q_HID), "b2": torch.zeros(1)}
            n["W1"][Q_HID - 1, Q_IN - 1] = 1.0
            n["W2"][0, Q_HID - 1] = 1.0
            nets.append(n)
    return nets


def make_quant_rows(kind, M, seed):
    """(X [M, 192], dq: three [M]).  "lin": X in [0, 3], dq in [-2, 2]; "one": X[M - 1][191] = 8 and dq[i][M - 1] = 1 alone."""
    if kind == "randn":
        return normal((M, Q_IN), seed), [normal((M,), seed + 1 + i) for i in range(3)]
    if kind == "lin":
        return _rint((M, Q_IN), 0, 3, seed), [ints((M,), 2, seed + 1 + i) for i in range(3)]
    X, dq = torch.zeros(M, Q_IN), [torch.zeros(M) for _ in range(3)]
    X[M - 1, Q_IN - 1] = 8.0
    for d in dq:
        d[M - 1] = 1.0
    return X, dq


def film_map(M, Mf, seed, one_sided=False):
    """(row_of [M], src_a [Mf], src_b [Mf]) int32 with every chain row named exactly once: M - Mf FiLM rows have both sides and a few more (none when
    one_sided), the others one side — a or b in turn — until the chain rows run out, the rest neither.  FiLM rows and chain rows are
    dealt in shuffled orders, so src_a / src_b do not increase."""
    assert 0 < Mf and M <= 2 * Mf and not (one_sided and M > Mf)
    g = _gen(seed)
    frows, crows = torch.randperm(Mf, generator=g).tolist(), torch.randperm(M, generator=g).tolist()
    both = 0 if one_sided else min(M // 2, max(M - Mf, 0) + max(1, Mf // 20))
    row_of, src_a, src_b = [-1] * M, [-1] * Mf, [-1] * Mf
    at = 0
    for j, q in enumerate(frows):
        if at >= M:
            break
        if j < both:
            src_a[q], src_b[q] = crows[at], crows[at + 1]
            row_of[crows[at]] = row_of[crows[at + 1]] = q
            at += 2
        else:
            (src_a if (j - both) % 2 == 0 else src_b)[q] = crows[at]
            row_of[crows[at]] = q
            at += 1
    assert at == M, (M, Mf, both)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    return i32(row_of), i32(src_a), i32(src_b)


def map_kinds(src_a, src_b):
    """Counts of FiLM rows with both sides, only a, only b, neither."""
    a, b = src_a >= 0, src_b >= 0
    return int((a & b).sum()), int((a & ~b).sum()), int((~a & b).sum()), int((~a & ~b).sum())


# ------------------------------------------------------------------------------------------------------------ case tables
# Launches use 512 threads = 8 waves; grid = min(256, max(n, ceil(ceil(rows n / 16) / 8))).
#   M 1 .. 129, n 3: one workgroup per network; M 17 with n 1, 2.
#   M 150: grid 4 dealt 2 / 1 / 1 (n 3), grid 3 dealt 2 / 1 (n 2): a grid that is no multiple of n.
#   M 4097 n 3: mid size, the largest exact probe.
#   M 11003 n 3: grid 256 dealt 86 / 85 / 85, ceil(11003 / 16) = 688 blocks > 85 * 8: the second round of the persistent loop.
#   M 32785 n 1: 2050 blocks > 256 * 8: the single-network second round and the deformation kernels'.
# (M, n_nets, exact probe too)
GEN_CASES = [(1, 3, True), (15, 3, True), (16, 3, True), (17, 3, True), (129, 3, True), (17, 1, True), (17, 2, True), (150, 3, True),
             (150, 2, True), (4097, 3, True), (11003, 3, False), (32785, 1, False)]
# (M, Mf, one-sided, exact probe too), n_nets = 3: FiLM rows with both sides, only a, only b, neither; Mf = 1; shuffled maps;
# (11003, 11003): the second round over FiLM blocks, every row one-sided
SHARED_CASES = [(2, 1, False, True), (17, 12, False, True), (150, 100, False, True), (4097, 2500, False, True), (11003, 11003, True, False)]
INFERENCE_M = [1, 17, 150, 4097]
INFERENCE_SHARED = {1: 1, 17: 12, 150: 100, 4097: 2500}      # M -> Mf of the shared run
QUANT_M = [1, 15, 16, 17, 4097, 32785]


# ------------------------------------------------------------------------------------------------------------ whole cases
def build_case(kind, M, n_nets, Mf=None, one_sided=False, acts=None, seed=0):
    """Everything one call pair needs, as fp32 CPU tensors: nets, deform, feat, cond [M, COND] (the chain rows' condition: the FiLM
    rows' gathered through row_of when they are shared), film (None, or cond [Mf, COND] / row_of / src_a / src_b), ys / gys (the
    backward probe: n_nets generators, then the deformation network)."""
    seed = seed + 7919 * M + 31 * n_nets + (Mf or 0)
    feat, cf = make_rows(kind, M, Mf or M, seed + 1)
    film = None
    if Mf:
        row_of, src_a, src_b = film_map(M, Mf, seed + 2, one_sided)
        if kind in ("one", "one_cond"):      # the one condition row that is not zero must be the last chain row's
            cf = torch.zeros_like(cf)
            cf[row_of[M - 1], COND - 1] = 2.0 if kind == "one" else 8.0
        film = {"cond": cf, "row_of": row_of, "src_a": src_a, "src_b": src_b}
    cond = cf if film is None else cf[film["row_of"].long()]
    nets = make_generators(kind, n_nets, seed + 1000, acts)
    ys, gys = backward_probe(kind, M, [n["out"] for n in nets] + [DEF_OUT], seed + 3)
    return {"nets": nets, "deform": make_deform(kind, seed + 2000), "feat": feat, "cond": cond, "film": film, "ys": ys, "gys": gys}


def cast(x, dtype, device=None):
    """x with every floating tensor in it cast (integer tensors — the maps — and plain numbers are kept, tensors moved)."""
    if torch.is_tensor(x):
        return x.to(device=device, dtype=dtype) if x.is_floating_point() else x.to(device=device)
    if isinstance(x, dict):
        return {k: cast(v, dtype, device) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(cast(v, dtype, device) for v in x)
    return x


def values(o):
    """{name: value} of a statement's {name: (value, scale, L)}."""
    return {k: v[0] for k, v in o.items()}


EXACT_ACTS = {1: (ACT_SIGMOID,), 2: (ACT_TANH, ACT_NONE), 3: (ACT_SIGMOID, ACT_NONE, ACT_TANH)}      # the exact backward probe's activations
