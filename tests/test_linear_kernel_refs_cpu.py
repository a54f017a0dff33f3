"""The references of tests/_linear_kernel_refs.py pinned on their own, without a GPU: a wrong reference must not be able to bless a
wrong kernel.  In float64 every epilogue's value against torch.nn.functional, every gradient-type epilogue against torch.autograd
of the forward it belongs to, wgrad_ref against autograd of F.linear, all to 1e-13; and the integer generators of the exact probes
of tests/test_linear_kernels_gpu.py: for every listed shape the sum of the ABSOLUTE terms of every output stays below 2^24, so the
float64 result and every partial sum, in any order, are integers fp32 holds exactly: the condition of the bit-for-bit claims.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import _linear_kernel_refs as R

TOL = 1e-13
f64 = torch.float64


def _close(a, b):
    return float((a - b).abs().max()) <= TOL * max(1.0, float(b.abs().max()))


def _data(M=37, K=29, N=23, seed=5):
    X, W, b, a1, a2 = (t.to(f64) for t in R.layer_inputs("randn", M, K, N, False, seed))
    return X, W, b, a1, a2


def test_linear_ref_both_layouts_and_scale():
    X, W, b, _, _ = _data()
    v, A = R.linear_ref(X, W, b, False)
    assert _close(v, F.linear(X, W, b))
    vt, At = R.linear_ref(X, W.t().contiguous(), b, True)
    assert torch.equal(v, vt) and torch.equal(A, At)
    # A: the sum of the absolute terms, term by term
    terms = (X[:, None, :] * W[None, :, :]).abs().sum(2) + b.abs()
    assert _close(A, terms) and bool((A >= v.abs() - 1e-12).all())
    v0, A0 = R.linear_ref(X, W, None, False)
    assert _close(v0, X @ W.t()) and _close(A0, A - b.abs())
    # fp32 in, fp32 out: the same function is the fp32 statement
    assert R.linear_ref(X.float(), W.float(), b.float())[0].dtype == torch.float32


def test_value_epilogues_match_torch_functional():
    X, W, b, a1, a2 = _data()
    v, _ = R.linear_ref(X, W, b)
    v = v * 0.3          # O(1): where the activations bend
    assert torch.equal(R.epilogue_ref(R.NONE, v)[0], v)
    assert torch.equal(R.epilogue_ref(R.RELU, v)[0], F.relu(v))
    y, y2, y3 = R.epilogue_ref(R.GELU_DUAL, v)
    assert torch.equal(y, v) and _close(y2, F.gelu(v)) and y3 is None
    assert _close(R.epilogue_ref(R.TANH, v)[0], torch.tanh(v))
    assert _close(R.epilogue_ref(R.SIGMOID, v)[0], torch.sigmoid(v))
    assert _close(R.epilogue_ref(R.ADD, v, a1)[0], v + a1)
    y, y2, y3 = R.epilogue_ref(R.FILM, v, a1, a2)
    assert torch.equal(y, v) and _close(y2, v * a1 + a2) and y3 is None
    for code in range(10):
        out = R.epilogue_ref(code, v, a1, a2)
        assert (out[1] is not None) == (code in R.HAS_Y2) and (out[2] is not None) == (code in R.HAS_Y3)
        sc = R.epilogue_scale(code, v.abs() + 1, a1, a2)
        assert all((s is None) == (o is None) for s, o in zip(sc, out))
    with pytest.raises(ValueError):
        R.epilogue_ref(10, v)


def test_gradient_epilogues_match_autograd():
    X, W, b, a1, a2 = _data()
    g = R.linear_ref(X, W, b)[0] * 0.3          # the upstream gradient: what the dX product delivers as v
    # MUL_GELU_GRAD: the input gradient of gelu at the pre-activation aux1
    z = a1.clone().requires_grad_(True)
    (dz,) = torch.autograd.grad(F.gelu(z), z, g)
    assert _close(R.epilogue_ref(R.MUL_GELU_GRAD, g, a1)[0], dz)
    # MUL_RELU_MASK: that of relu, the mask taken from relu's OUTPUT (aux1 = relu(z) > 0 iff z > 0)
    z = a1.clone().requires_grad_(True)
    out = F.relu(z)
    (dz,) = torch.autograd.grad(out, z, g)
    assert torch.equal(R.epilogue_ref(R.MUL_RELU_MASK, g, out.detach())[0], dz)
    # FILM_GRAD: the three gradients of gamma * h + beta (aux1 = h, aux2 = gamma)
    gamma, h, beta = (t.clone().requires_grad_(True) for t in (a2, a1, torch.zeros_like(a1)))
    d_gamma, d_h, d_beta = torch.autograd.grad(gamma * h + beta, (gamma, h, beta), g)
    y, y2, y3 = R.epilogue_ref(R.FILM_GRAD, g, a1, a2)
    assert _close(y, d_beta) and _close(y2, d_gamma) and _close(y3, d_h)
    # gelu_grad on its own, far tails included
    z = torch.linspace(-9, 9, 721, dtype=f64).requires_grad_(True)
    (dz,) = torch.autograd.grad(F.gelu(z).sum(), z)
    assert _close(R.gelu_grad(z.detach()), dz)


def test_wgrad_accumulate_shared_match_autograd():
    G, X = (t.to(f64) for t in R.wgrad_inputs("randn", 41, 23, 29, 3))
    W, b = torch.zeros(23, 29, dtype=f64, requires_grad=True), torch.zeros(23, dtype=f64, requires_grad=True)
    dW_a, db_a = torch.autograd.grad(F.linear(X, W, b), (W, b), G)
    dW, db, sW, sb = R.wgrad_ref(G, X)
    assert _close(dW, dW_a) and _close(db, db_a)
    assert _close(sW, (G.abs()[:, :, None] * X.abs()[:, None, :]).sum(0)) and _close(sb, G.abs().sum(0))
    jobs = [(x.to(f64), w.to(f64)) for x, w in R.accum_inputs("randn", 19, (2, 50, 66), 37, 1)]
    Y, A = R.accumulate_ref(jobs)
    assert _close(Y, sum(x @ w for x, w in jobs)) and _close(A, sum(x.abs() @ w.abs() for x, w in jobs))
    Xs, sj = R.shared_inputs("randn", 19, 100, (1, 12, 50), 2)
    Xs, sj = Xs.to(f64), [(w.to(f64), bb.to(f64)) for w, bb in sj]
    for (y, y2, a), (w, bb) in zip(R.shared_input_ref(Xs, sj), sj):
        assert _close(y, F.linear(Xs, w, bb)) and _close(y2, F.gelu(F.linear(Xs, w, bb))) and _close(a, Xs.abs() @ w.abs().t() + bb.abs())


# --------------------------------------------------------------------------------------------- the exact probes' generators
def _integers(t, bound):
    return bool((t == t.round()).all()) and float(t.abs().max()) <= bound


def _below(worst, *scales):
    m = max(float(s.max()) for s in scales if s is not None)
    assert m < R.EXACT_LIMIT, m
    return max(worst, m)


def test_integer_generators_stay_exact_layers():
    """Every (K, N, M) of the layer cases, both weight layouts, every exact epilogue: sum of absolute terms < 2^24."""
    worst = 0.0
    shapes = [(K, N, M) for K, N in R.LAYER_SHAPES for M in R.LAYER_M + R.LAYER_M_MORE.get((K, N), [])]
    shapes += [(R.EPI_K, N, M) for N in R.EPI_N for M in R.EPI_M] + [(K, N, M) for K, N in R.EPI_1024 for M in R.EPI_M]
    shapes += [(K, N, R.ALIGN_M) for K, N in R.ALIGN_SHAPES]
    for K, N, M in shapes:
        for wio in (False, True):
            X, W, b, a1, a2 = R.layer_inputs("int", M, K, N, wio, 1000 + K + N)
            assert all(_integers(t, 4) for t in (X, W, b, a1, a2)) and X.dtype == torch.float32
            _, A = R.linear_ref(X.double(), W.double(), b.double(), wio)
            for code in R.EXACT_EPILOGUES:
                worst = _below(worst, *R.epilogue_scale(code, A, a1.double(), a2.double()))
    if R.PRINT:
        print(f"LINEAR_INT layers: largest sum of absolute terms {worst:.0f} (2^24 = {R.EXACT_LIMIT:.0f})")
    # the worst case in closed form: 192 terms of 4 * 4, a bias of 4, FiLM's factor 4 and shift 4
    assert worst <= (192 * 16 + 4) * 4 + 4


def test_integer_generators_stay_exact_many():
    worst = 0.0
    for Ks, N, M in R.ACCUM_CASES:
        jobs = R.accum_inputs("int", M, Ks, N, 7)
        assert all(_integers(x, 4) and _integers(w, 4) for x, w in jobs)
        worst = _below(worst, R.accumulate_ref([(x.double(), w.double()) for x, w in jobs])[1])
    for K, Ns, M in R.SHARED_CASES:
        X, jobs = R.shared_inputs("int", M, K, [n for n, _ in Ns], 9)
        assert _integers(X, 4) and all(_integers(w, 4) and _integers(b, 4) for w, b in jobs)
        worst = _below(worst, *[a for _, _, a in R.shared_input_ref(X.double(), [(w.double(), b.double()) for w, b in jobs])])
    if R.PRINT:
        print(f"LINEAR_INT accumulate / shared input: largest sum of absolute terms {worst:.0f}")
    assert worst <= 8 * 192 * 16


def test_integer_generators_stay_exact_wgrad():
    """G in [-2, 2], X in [-4, 4] up to 4097 rows; G in {-1, 0, 1} at 70001 rows."""
    worst = 0.0
    for N, K in R.WGRAD_SHAPES:
        G, X = R.wgrad_inputs("int", max(R.WGRAD_M), N, K, 100 + N + K)
        assert _integers(G, 2) and _integers(X, 4)
        _, _, sW, sb = R.wgrad_ref(G.double(), X.double())
        worst = _below(worst, sW, sb)          # fewer rows are a prefix-sized subset of these terms: the bound only shrinks
    assert worst <= 4097 * 8
    for N, K in R.WGRAD_BIG_SHAPES:
        G, X = R.wgrad_inputs("int", R.WGRAD_M_BIG, N, K, 100 + N + K, g_bound=1)
        assert _integers(G, 1) and _integers(X, 4)
        _, _, sW, sb = R.wgrad_ref(G.double(), X.double())
        worst = _below(worst, sW, sb)
    if R.PRINT:
        print(f"LINEAR_INT weight gradients: largest sum of absolute terms {worst:.0f}")
    assert worst <= 70001 * 4


def test_single_element_probe_reaches_one_output():
    X, W, b, a1, a2 = R.layer_inputs("one", 17, 51, 37, False, 0)
    v, _ = R.linear_ref(X.double(), W.double(), b.double())
    assert int((v != 0).sum()) == 1 and float(v[16, 36]) == 6.0
    X, W, b, a1, a2 = R.layer_inputs("one", 17, 51, 37, True, 0)
    v, _ = R.linear_ref(X.double(), W.double(), b.double(), True)
    assert int((v != 0).sum()) == 1 and float(v[16, 36]) == 6.0
    G, X = R.wgrad_inputs("one", 17, 23, 19, 0)
    dW, db, _, _ = R.wgrad_ref(G.double(), X.double())
    assert int((dW != 0).sum()) == 1 and float(dW[22, 18]) == 6.0 and int((db != 0).sum()) == 1 and float(db[22]) == 2.0
    Y, _ = R.accumulate_ref([(x.double(), w.double()) for x, w in R.accum_inputs("one", 17, (2, 50), 37, 0)])
    assert int((Y != 0).sum()) == 1 and float(Y[16, 36]) == 6.0
