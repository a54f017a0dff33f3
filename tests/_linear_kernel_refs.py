"""Plain tensor statements of the MFMA layer kernels (csrc/linear.hip, linear_ws.h, linear_epi_{a,b,c,d}.hip, linear_accum.hip) and of
the weight gradients (csrc/linear_wgrad.hip), written from include/gsvc_hip.h.  Called with float64 tensors they are the references
of tests/test_linear_kernels_gpu.py; called with float32 tensors they are "the fp32 tensor statement" those tests calibrate against.
tests/test_linear_kernel_refs_cpu.py pins them, and the input generators and case tables below, without a GPU.  Nothing here imports
the package under test.

Every function returns, next to its value, the SCALE its error is taken on: the sum of the absolute terms of each output
(A = |X| |W|^T + |b| for a layer), so that an error reads in units of the output's own rounding, element by element.
"""
import math

import torch

from tests._loss_kernel_refs import EPS32, PRINT, err, err_each  # noqa: F401  (re-exported for the tests)

# epilogue codes of gsvc_linear_forward_ex (include/gsvc_hip.h)
NONE, RELU, GELU_DUAL, TANH, SIGMOID, MUL_GELU_GRAD, MUL_RELU_MASK, FILM, FILM_GRAD, ADD = range(10)
EPI_NAMES = ("none", "relu", "gelu_dual", "tanh", "sigmoid", "mul_gelu_grad", "mul_relu_mask", "film", "film_grad", "add")
NEEDS_AUX1 = (MUL_GELU_GRAD, MUL_RELU_MASK, FILM, FILM_GRAD, ADD)
NEEDS_AUX2 = (FILM, FILM_GRAD)
HAS_Y2 = (GELU_DUAL, FILM, FILM_GRAD)
HAS_Y3 = (FILM_GRAD,)
EXACT_EPILOGUES = (NONE, RELU, ADD, MUL_RELU_MASK, FILM, FILM_GRAD, GELU_DUAL)      # GELU_DUAL: its pre-activation Y only
TRANSCENDENTAL = (TANH, SIGMOID, GELU_DUAL, MUL_GELU_GRAD)                           # GELU_DUAL: its Y2 only

EXACT_LIMIT = float(2 ** 24)      # integers below it, and their sums in any order, are exact in fp32


# ------------------------------------------------------------------------------------------------------------ statements
def linear_ref(X, W, b=None, w_in_out=False):
    """(v, A): v = X W^T + b for W [N, K] (X W for w_in_out, W [K, N]); A = |X| |W|^T + |b|."""
    Wt = W if w_in_out else W.t()
    v, A = X @ Wt, X.abs() @ Wt.abs()
    if b is not None:
        v, A = v + b, A + b.abs()
    return v, A


def gelu(z):
    """GELU in erf form: z Phi(z)."""
    return 0.5 * z * (1.0 + torch.erf(z * (1.0 / math.sqrt(2.0))))


def gelu_grad(z):
    """GELU'(z) = Phi(z) + z phi(z)."""
    cdf = 0.5 * (1.0 + torch.erf(z * (1.0 / math.sqrt(2.0))))
    pdf = torch.exp(-0.5 * z * z) * (1.0 / math.sqrt(2.0 * math.pi))
    return cdf + z * pdf


def epilogue_ref(code, v, aux1=None, aux2=None):
    """(Y, Y2, Y3) of gsvc_linear_forward_ex for the pre-epilogue value v; None for an output the epilogue does not have."""
    if code == NONE:
        return v, None, None
    if code == RELU:
        return torch.clamp_min(v, 0), None, None
    if code == GELU_DUAL:
        return v, gelu(v), None
    if code == TANH:
        return torch.tanh(v), None, None
    if code == SIGMOID:
        return 1.0 / (1.0 + torch.exp(-v)), None, None
    if code == MUL_GELU_GRAD:
        return v * gelu_grad(aux1), None, None
    if code == MUL_RELU_MASK:
        return torch.where(aux1 > 0, v, torch.zeros_like(v)), None, None
    if code == FILM:
        return v, v * aux1 + aux2, None
    if code == FILM_GRAD:
        return v, v * aux1, v * aux2
    if code == ADD:
        return v + aux1, None, None
    raise ValueError(code)


def epilogue_scale(code, A, aux1=None, aux2=None):
    """The scales of (Y, Y2, Y3): the sum of the absolute terms of each output; max(1, A) for an output that went through a
    transcendental function (it is O(1): its error is the function's own, not the product's)."""
    one = torch.clamp_min(A, 1.0)
    if code in (NONE, RELU, MUL_RELU_MASK):
        return A, None, None
    if code == GELU_DUAL:
        return A, one, None
    if code in (TANH, SIGMOID, MUL_GELU_GRAD):
        return one, None, None
    if code == FILM:
        return A, A * aux1.abs() + aux2.abs(), None
    if code == FILM_GRAD:
        return A, A * aux1.abs(), A * aux2.abs()
    if code == ADD:
        return A + aux1.abs(), None, None
    raise ValueError(code)


def wgrad_ref(G, X):
    """(dW, db, scale of dW, scale of db): dW = G^T X [N, K], db = column sums of G [N]; scales |G|^T |X| and the column sums of |G|."""
    return G.t() @ X, G.sum(0), G.abs().t() @ X.abs(), G.abs().sum(0)


def accumulate_ref(jobs):
    """(Y, A) = (sum_p X_p W_p, sum_p |X_p| |W_p|) for jobs [(X_p [M, K_p], W_p [K_p, N])]."""
    Y = A = None
    for X, W in jobs:
        v, a = linear_ref(X, W, None, True)
        Y, A = (v, a) if Y is None else (Y + v, A + a)
    return Y, A


def shared_input_ref(X, jobs):
    """[(Y_p, Y2_p, A_p)] for jobs [(W_p [N_p, K], b_p or None)]: Y_p = X W_p^T + b_p, Y2_p = GELU(Y_p)."""
    out = []
    for W, b in jobs:
        v, A = linear_ref(X, W, b, False)
        out.append((v, gelu(v), A))
    return out


# ------------------------------------------------------------------------------------------------------------ inputs
def ints(shape, bound, seed):
    """fp32 tensor of integers drawn uniformly from [-bound, bound], every element its own draw."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, tuple(shape), generator=gen).to(torch.float32)


def normal(shape, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(shape), generator=gen) * scale


def layer_inputs(kind, M, K, N, w_in_out, seed):
    """X [M, K], W ([N, K] or [K, N]), b [N], aux1, aux2 [M, N] on the CPU in fp32.  kind "int": integers in [-4, 4]; "randn": normal
    data with W scaled by 1 / sqrt(K), so that v is O(1) and the activations are exercised where they bend; "one": all zeros
    but X[M - 1, K - 1] = 3 and W[n = N - 1, k = K - 1] = 2 (the last row, the last k and the last column: only Y[M - 1, N - 1]
    = 6 may be non-zero)."""
    wshape = (K, N) if w_in_out else (N, K)
    if kind == "int":
        return (ints((M, K), 4, seed), ints(wshape, 4, seed + 1), ints((N,), 4, seed + 2), ints((M, N), 4, seed + 3),
                ints((M, N), 4, seed + 4))
    if kind == "randn":
        return (normal((M, K), seed), normal(wshape, seed + 1, K ** -0.5), normal((N,), seed + 2, 0.5), normal((M, N), seed + 3),
                normal((M, N), seed + 4))
    assert kind == "one"
    X, W = torch.zeros(M, K), torch.zeros(wshape)
    X[M - 1, K - 1] = 3.0
    W[(K - 1, N - 1) if w_in_out else (N - 1, K - 1)] = 2.0
    return X, W, torch.zeros(N), torch.ones(M, N), torch.zeros(M, N)


def wgrad_inputs(kind, M, N, K, seed, g_bound=2):
    """G [M, N], X [M, K].  "int": G in [-g_bound, g_bound], X in [-4, 4]; "randn"; "one": G[M - 1, N - 1] = 2 and
    X[M - 1, K - 1] = 3 alone (only dW[N - 1, K - 1] = 6 and db[N - 1] = 2 may be non-zero)."""
    if kind == "int":
        return ints((M, N), g_bound, seed), ints((M, K), 4, seed + 1)
    if kind == "randn":
        return normal((M, N), seed), normal((M, K), seed + 1)
    assert kind == "one"
    G, X = torch.zeros(M, N), torch.zeros(M, K)
    G[M - 1, N - 1] = 2.0
    X[M - 1, K - 1] = 3.0
    return G, X


def accum_inputs(kind, M, Ks, N, seed):
    """[(X_p [M, K_p], W_p [K_p, N])]; "one": only the last product's X[M - 1, K - 1] and W[K - 1, N - 1] are non-zero."""
    jobs = []
    for p, K in enumerate(Ks):
        if kind == "one" and p < len(Ks) - 1:
            jobs.append((torch.zeros(M, K), torch.zeros(K, N)))
        else:
            jobs.append(tuple(layer_inputs(kind, M, K, N, True, seed + 10 * p)[:2]))
    return jobs


def shared_inputs(kind, M, K, Ns, seed):
    """(X [M, K], [(W_p [N_p, K], b_p [N_p])])."""
    X = layer_inputs(kind, M, K, 1, False, seed)[0]
    return X, [tuple(layer_inputs(kind, 1, K, N, False, seed + 10 * (p + 1))[1:3]) for p, N in enumerate(Ns)]


# ------------------------------------------------------------------------------------------------------------ case tables
# (K, N) of k_linear_ws with the path each reaches for 16-byte aligned X and Y: load width VEC (K % 4), store width sv (N % 4),
# NT = ceil(N / 16) column tiles, KGM = ceil(K / 16) rounded up to even, and the workgroup size launch_ws3 picks for the plain
# (non-epilogue) kernel: 1024 threads iff NT + KGM <= (VEC 4: 15, VEC 2: 13, VEC 1: 10) - (2 if NT > 8), from
# NT * 4 + KGM * 4 <= (60 | 52 | 40) - (8 if NT > 8).
LAYER_SHAPES = [
    (3, 1),          # VEC 1 sv 1  NT 1  KGM 2   1024   smallest tile
    (16, 16),        # VEC 4 sv 4  NT 1  KGM 2   1024   one 16 x 16 tile
    (17, 23),        # VEC 1 sv 1  NT 2  KGM 2   1024   odd K and N
    (51, 37),        # VEC 1 sv 1  NT 3  KGM 4   1024
    (50, 100),       # VEC 2 sv 4  NT 7  KGM 4   1024
    (100, 70),       # VEC 4 sv 2  NT 5  KGM 8   1024   (5 + 8 = 13 <= 15)
    (100, 10),       # VEC 4 sv 2  NT 1  KGM 8   1024   thin output
    (66, 66),        # VEC 2 sv 2  NT 5  KGM 6   1024   (11 <= 13)
    (116, 100),      # VEC 4 sv 4  NT 7  KGM 8   1024   (15 <= 15) mlp_deform's first layer
    (130, 82),       # VEC 2 sv 2  NT 6  KGM 10  512    (16 > 13)
    (177, 33),       # VEC 1 sv 1  NT 3  KGM 12  512    (15 > 10)
    (150, 192),      # VEC 2 sv 4  NT 12 KGM 10  512
    (192, 150),      # VEC 4 sv 2  NT 10 KGM 12  512
    (192, 192),      # VEC 4 sv 4  NT 12 KGM 12  512    largest supported
]
LAYER_M = [1, 15, 16, 17, 257]
LAYER_M_MORE = {(50, 100): [63, 64, 65, 1025, 4097], (17, 23): [63, 64, 65, 1025, 4097],
                # a workgroup's second round of the persistent loop needs more than 256 * WAVES row blocks: 16 waves (1024 threads)
                # -> M > 65536, 8 waves (512 threads) -> M > 32768
                (16, 16): [65536 + 17], (130, 82): [32768 + 17]}
# the epilogue kernels hold 36 more registers: 1024 threads iff VEC 4 and NT + KGM <= 6, so every K = 66 case below takes 512
# threads; (16, 16) and (32, 64) are the smallest shapes that give the epilogue kernels their 1024-thread side (NT 1 / 4, KGM 2)
EPI_K = 66
EPI_N = [10, 37, 70, 100, 150, 192]      # translation units a (10, 37), b (70, 100), c (150), d (192); sv 2, 1, 2, 4, 2, 4
EPI_M = [17, 257]
EPI_1024 = [(16, 16), (32, 64)]
ALIGN_SHAPES = [(100, 100), (50, 100)]
ALIGN_M = 257

ACCUM_CASES = [      # (Ks, N, M): n_jobs 1, 2, 8; K_p from {2, 50, 66, 100, 192}; the scalar (N % 4 != 0) and float4 weight staging
    ((2,), 1, 1), ((50,), 37, 17), ((192,), 192, 4097), ((100,), 100, 65536),
    ((66, 2), 37, 4097), ((192, 50), 100, 17), ((100, 66), 192, 1), ((2, 50), 1, 65536),
    ((2, 50, 66, 100, 192, 100, 66, 50), 100, 17), ((192, 100, 66, 50, 2, 192, 100, 66), 192, 4097),
    ((50, 50, 2, 2, 66, 66, 100, 192), 37, 1), ((2, 50, 66, 100, 192, 2, 50, 66), 1, 4097),
    ((66, 100, 2, 50, 192, 66, 100, 2), 100, 65536),
]
SHARED_CASES = [     # (K, [(N_p, wants Y2)], M): n_jobs 1, 3, 8; K in {4, 100, 192}; N_p from {1, 12, 50, 100, 160}
    (4, [(1, True)], 1), (100, [(160, False)], 17), (192, [(50, True)], 4097), (4, [(12, False)], 65536),
    (100, [(1, False), (50, True), (160, True)], 4097), (192, [(12, True), (100, False), (1, True)], 17),
    (4, [(160, True), (12, False), (100, True)], 1), (100, [(12, True), (1, False), (50, False)], 65536),
    (192, [(1, True), (12, False), (50, True), (100, False), (160, True), (50, False), (12, True), (1, False)], 4097),
    (100, [(160, False), (100, True), (50, False), (12, True), (1, False), (160, True), (100, False), (50, True)], 17),
    (4, [(1, False), (12, True), (50, False), (100, True), (160, False), (1, True), (12, False), (50, True)], 1),
    (192, [(12, False), (1, True), (12, True), (1, False), (50, True), (12, False), (1, True), (50, False)], 65536),
]

# (N, K) of the weight gradients.  wgrad_launch (16-byte aligned rows of a width that is a multiple of 4: at most 4 tiles per
# block, else 3): bn_t = ceil(ceil(N / 16) / mt_g), bk_t likewise; k_linear_wgrad_t iff bn_t * bk_t <= 12 and the blocks fit LDS.
WGRAD_SHAPES = [(1, 50), (10, 100), (23, 17), (30, 100), (49, 81), (66, 66), (70, 100), (100, 50), (100, 100), (100, 116), (129, 33),
                (82, 130), (192, 150),
                (192, 192),      # 12 tiles / 4 = 3 blocks a side: 9 wave pairs, RS 1 (alone in a batch: 12 % 9 != 0)
                # 177 is odd: vec_of gives 1 for G and X, so mt_g = mt_x = 3 and bn_t = bk_t = ceil(12 / 3) = 4: 16 blocks > 12 waves
                # -> launch_wgrad2<1, 1> with 64 x 64 blocks: BN = BK = 3, 9 waves, RS 1, 9 * 16 KiB = 144 KiB of LDS
                (177, 177)]
WGRAD_M = [1, 15, 16, 17, 100, 4097]
WGRAD_M_BIG = 70001      # for (100, 100) and (23, 17); the exact probe there draws G from {-1, 0, 1}
WGRAD_BIG_SHAPES = [(100, 100), (23, 17)]
