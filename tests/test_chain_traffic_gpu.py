"""Shared FiLM rows in the generators' backward (csrc/mlp_chain.hip): k_trunk_bwd walks FiLM rows and takes the two chain rows
behind each one through the chain together, so the FiLM networks' backward receives the two views' summed d gamma / d beta —
one row per FiLM row — and the per-view rows of them never exist.  Everything a chain row produces must keep its bits (the
same operands in the same order; only the order in which rows are visited differs); the FiLM networks' own gradients, which
now start from the sums, are held against float64.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

M_ROWS = 6001            # the smallest ragged size above mlp.MIN_ROWS (odd row count, partial last 16-row block)
FILM_ROWS = 3700         # 231 whole 16-row blocks of FiLM rows and a last one of 4
EMPTY = (160, 208)       # FiLM rows nobody sees: three whole 16-row blocks in a row


def _hand_built_film(M, Mf):
    """(kinds, row_of, src_a, src_b): FiLM rows of all four kinds — 0 both views, 1 view a only, 2 view b only, 3 neither — with
    a run of rows nobody sees; view a's chain rows come first, each view's in increasing FiLM row order (as gsvc_film_row_maps
    leaves them), every chain row named exactly once."""
    rng = np.random.default_rng(M)
    kinds = rng.choice(4, size=Mf, p=[0.68, 0.14, 0.14, 0.04])
    kinds[EMPTY[0]:EMPTY[1]] = 3
    kinds[Mf - 4:] = [0, 1, 2, 3]                      # the ragged last block holds one of each
    free = np.r_[0:EMPTY[0], EMPTY[1]:Mf - 4]

    def sides():
        return 2 * int((kinds == 0).sum()) + int((kinds == 1).sum()) + int((kinds == 2).sum())
    for q in free[::-1]:                                # bring the number of (view, anchor) rows to M exactly, one at a time
        n = sides()
        if n == M:
            break
        if n < M and kinds[q] != 0:
            kinds[q] = 1 if kinds[q] == 3 else 0
        elif n > M and kinds[q] != 3:
            kinds[q] = 1 if kinds[q] == 0 else 3
    assert sides() == M and all((kinds == k).sum() > 20 for k in range(4))
    has_a, has_b = (kinds == 0) | (kinds == 1), (kinds == 0) | (kinds == 2)
    in_a, in_b = np.nonzero(has_a)[0], np.nonzero(has_b)[0]
    na = len(in_a)
    src_a, src_b = np.full(Mf, -1, np.int32), np.full(Mf, -1, np.int32)
    src_a[in_a] = np.arange(na, dtype=np.int32)
    src_b[in_b] = np.arange(na, M, dtype=np.int32)
    row_of = np.concatenate([in_a, in_b]).astype(np.int32)
    return kinds, row_of, src_a, src_b


def _networks():
    from gsvc_amd.model import GeluSequential, GeneratorNet, Linear
    torch.manual_seed(M_ROWS)
    gens = [GeneratorNet(50, 10, 100, 66, out_act=torch.nn.Tanh()).cuda(), GeneratorNet(50, 30, 100, 66, out_act=torch.nn.Sigmoid()).cuda(),
            GeneratorNet(50, 70, 100, 66).cuda()]
    deform = GeluSequential(Linear(116, 100), torch.nn.GELU(), Linear(100, 100), torch.nn.GELU(), Linear(100, 100), torch.nn.GELU(),
                            Linear(100, 100), torch.nn.GELU(), Linear(100, 30)).cuda()
    return gens, deform


def _generator_f64(p64, act, feat, cond):
    """The generator in float64 on its fourteen parameters in mlp.GEN_FIELDS order (leaves that collect the gradient)."""
    w1, b1, w2, b2, w3, b3, wg0, bg0, wg1, bg1, wb0, bb0, wb1, bb1 = p64
    h = F.linear(F.gelu(F.linear(feat, w1, b1)), w2, b2)
    gamma = F.linear(torch.relu(F.linear(cond, wg0, bg0)), wg1, bg1)
    beta = F.linear(torch.relu(F.linear(cond, wb0, bb0)), wb1, bb1)
    y = F.linear(gamma * h + beta, w3, b3)
    return act(y) if act is not None else y


def _trunk_weight_gradients(feat, cond, film, plist, acts, gs):
    """gsvc_generate_all_forward / _backward through the C-ABI with the FiLM networks' gradient pointers NULL (a NULL weight
    pointer skips that layer's product): the generators' batched weight-gradient launch then holds the W1..W3 products alone, all
    of them over the M chain rows, so its workgroups — and with them the order of every sum — are dealt the same way with and
    without shared FiLM rows.  (Inside a full backward the FiLM products, over Mf or M rows, share that launch and shift the split.)
    Returns the gradients (generators' W1 b1 W2 b2 W3 b3 x 3, then mlp_deform's) and the feature gradient."""
    from gsvc_amd import _lib, mlp
    L, M = _lib.lib(), feat.shape[0]
    outs, saved = mlp._chain_forward(feat, cond, acts, film, plist, keep=True)
    grads = [torch.full_like(p, float("nan")) for p in plist]
    nets, dd, film_p, Mf, gds, gd = mlp._chain_desc(plist, acts, film, grads)
    for g in range(3):
        for name in mlp.GEN_FIELDS[6:]:
            setattr(gds[g], name, None)
    floats = sum((int(L.gsvc_generator_scratch_floats(C.byref(nets[g]), M, Mf)) + 3) // 4 * 4 for g in range(3))
    scratch = torch.empty(floats, device="cuda")
    scratch_d = torch.empty(int(L.gsvc_deform_scratch_floats(C.byref(dd), M)), device="cuda")
    gfeat = [torch.full((M, 50), float("nan"), device="cuda") for _ in range(4)]
    _lib.check(L.gsvc_generate_all_backward(nets, 3, C.byref(dd), feat.data_ptr(), cond.data_ptr(), M, film_p, mlp._ptr_array(saved),
                                            mlp._ptr_array(outs[:3]), mlp._ptr_array(gs), scratch.data_ptr(), scratch_d.data_ptr(),
                                            gfeat[3].data_ptr(), mlp._ptr_array(gfeat[:3]), gds, C.byref(gd), _lib.current_stream(feat.device), None),
               "gsvc_generate_all_backward")
    torch.cuda.synchronize()
    keep = [g for i in range(3) for g in grads[14 * i:14 * i + 6]] + grads[42:]
    return keep, gfeat[3]


def test_paired_backward_equals_unpaired_bit_for_bit():
    """mlp.generate_all at M = 6001 with a hand-built film (FiLM rows of all four kinds: both views, a only, b only, neither; 48
    consecutive rows nobody sees = whole empty 16-row blocks; a ragged last FiLM block) against the same call with film=None on
    the gathered condition: the four outputs, the feature gradient, every W1..W3 / b1..b3 gradient of the generators and every
    mlp_deform gradient have the same bits (the generators' through the C-ABI, see _trunk_weight_gradients).  The generators'
    gradients of the shared run — the FiLM networks' sums run over FiLM rows, in another order than the unshared run's — against
    a float64 evaluation at 1e-3 of the gradient's scale (the project's gradient tolerance); bg1 / bb1 are the column sums of the
    summed d gamma / d beta the trunk backward now writes.  Rows whose first-layer FiLM pre-activation lies within 1e-4 of the
    ReLU's kink take no part (their gy is zero), as in test_mlp_gpu."""
    from gsvc_amd import mlp
    M, Mf = M_ROWS, FILM_ROWS
    kinds, row_of, src_a, src_b = _hand_built_film(M, Mf)
    assert (kinds[EMPTY[0]:EMPTY[1]] == 3).all() and EMPTY[1] - EMPTY[0] >= 40 and EMPTY[0] % 16 == 0 and Mf % 16 != 0
    gens, deform = _networks()
    lin = list(deform)[0::2]
    gen_ = torch.Generator(device="cuda").manual_seed(7)
    feat = (torch.randn(M, 50, device="cuda", generator=gen_) * 2).requires_grad_(True)
    cond_film = torch.randn(Mf, 66, device="cuda", generator=gen_)
    film = (cond_film, *(torch.from_numpy(a).cuda() for a in (row_of, src_a, src_b)))
    cond = cond_film.index_select(0, film[1].long())
    gs = [torch.randn(M, n, device="cuda", generator=gen_) for n in (10, 30, 70, 30)]
    with torch.no_grad():
        bad = torch.zeros(M, dtype=torch.bool, device="cuda")
        for net in gens:
            f = net.film
            pre = torch.cat([F.linear(cond, f.fc_gamma0.weight, f.fc_gamma0.bias), F.linear(cond, f.fc_beta0.weight, f.fc_beta0.bias)], 1)
            bad |= (pre.abs() < 1e-4).any(dim=1)
        for g in gs[:3]:
            g[bad] = 0
    assert mlp.chain_usable(feat, cond, gens, lin)
    params = [p for net in gens for p in mlp._generator_params(net)] + [p for l in lin for p in (l.weight, l.bias)]      # mlp.generate_all's order

    def run(film_):
        feat.grad = None
        for p in params:
            p.grad = None
        outs = mlp.generate_all(gens, lin, feat, cond, film=film_)
        assert "GenerateAll" in type(outs[0].grad_fn).__name__
        sum((o * g).sum() for o, g in zip(outs, gs)).backward()
        return [o.detach() for o in outs], feat.grad.clone(), [p.grad.clone() for p in params]
    o_s, gf_s, gp_s = run(film)
    o_u, gf_u, gp_u = run(None)
    for a, b in zip(o_s, o_u):
        assert torch.equal(a, b)
    assert torch.equal(gf_s, gf_u)
    deform_ids = {id(p) for p in deform.parameters()}
    for p, a, b in zip(params, gp_s, gp_u):
        if id(p) in deform_ids:
            assert torch.equal(a, b), tuple(p.shape)
    # W1..W3 / b1..b3 of the generators: their products share one launch with the FiLM networks' (Mf rows here, M there), and the
    # launch deals its workgroups by the products' work, so inside a full backward the two runs split the rows differently.  With
    # the FiLM products left out the split is the same and the gradients have the same bits
    plist = [p.detach().contiguous() for p in params]
    acts = tuple(mlp._act_code(n) for n in gens)
    tw_s, tf_s = _trunk_weight_gradients(feat.detach(), cond.contiguous(), film, plist, acts, gs)
    tw_u, tf_u = _trunk_weight_gradients(feat.detach(), cond.contiguous(), None, plist, acts, gs)
    assert len(tw_s) == 3 * 6 + 10 and torch.equal(tf_s, tf_u) and torch.equal(tf_s, gf_s)
    for a, b in zip(tw_s, tw_u):
        assert not torch.isnan(a).any() and torch.equal(a, b), tuple(a.shape)
    for a, b in zip(tw_s[18:], [g for p, g in zip(params, gp_s) if id(p) in deform_ids]):
        assert torch.equal(a, b)
    # the generators' gradients of the shared run — the FiLM networks' start from the summed d gamma / d beta — against float64
    feat64, cond64 = feat.detach().double(), cond.double()
    for i, (net, g) in enumerate(zip(gens, gs)):
        p64 = [p.detach().double().requires_grad_(True) for p in mlp._generator_params(net)]
        (_generator_f64(p64, net.out_act, feat64, cond64) * g.double()).sum().backward()
        for name, got, ref in zip(mlp.GEN_FIELDS, gp_s[14 * i:14 * (i + 1)], p64):
            scale = max(1e-6, ref.grad.abs().max().item())
            err = (got.double() - ref.grad).abs().max().item()
            assert err <= 1e-3 * scale, (i, name, err, scale)


def test_generator_scratch_shrinks_with_shared_film_rows():
    """gsvc_generator_scratch_floats: with shared FiLM rows d gamma / d beta exist once per FiLM row only, so against the size
    without them (every per-FiLM-row tensor — d gamma, d beta and the FiLM hidden layers' gradients gcg, gcb [COND] — once per chain
    row) the scratch is smaller by (2 HID + 2 COND) (M - Mf) floats: 2 HID (M - Mf) for d gamma / d beta, the rest for gcg / gcb,
    which already lived per FiLM row.  Each of the seven regions starts on a multiple of 4 floats inside a fixed allowance, so the
    two sizes differ by exactly that."""
    from gsvc_amd import _lib
    L = _lib.lib()
    HID, COND = 100, 66
    for out in (10, 30, 70):
        d = _lib.GeneratorNetC()
        d.feat_dim, d.cond_dim, d.hidden_dim, d.out_dim, d.out_act = 50, COND, HID, out, 0
        for M, Mf in ((6001, 3700), (195_000, 106_000), (4096, 4096)):
            plain, shared = int(L.gsvc_generator_scratch_floats(C.byref(d), M, 0)), int(L.gsvc_generator_scratch_floats(C.byref(d), M, Mf))
            assert plain - shared == (2 * HID + 2 * COND) * (M - Mf)
            assert plain - shared >= 2 * HID * (M - Mf)
            # per chain row: go [out], gh, gz1 [HID] and nothing else
            more = int(L.gsvc_generator_scratch_floats(C.byref(d), M + 16, Mf))
            assert more - shared == 16 * (d.out_dim + 2 * HID)
