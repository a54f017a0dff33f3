"""The MFMA layer kernels (csrc/linear.hip, linear_ws.h, linear_epi_{a,b,c,d}.hip, linear_accum.hip) and the weight gradients
(csrc/linear_wgrad.hip) through their C entry points, at the row counts, widths, alignments and job mixes that choose between their
code paths, each against the float64 run of its plain tensor statement in tests/_linear_kernel_refs.py.  No module of the package
stands between the test and the kernel, so nothing here can fall back to torch.

Two assertions per shape:
  * exact probe: integer inputs whose sums of absolute terms stay below 2^24 (tests/test_linear_kernel_refs_cpu.py shows it for
    every case table used here), so the fp32 result equals the float64 result bit for bit in whatever order the kernel sums; plus a
    run with a single non-zero product, which pins the output it reaches;
  * float64 rule: normal data, e_kernel <= 4 * e32 + 4 * eps32, both errors max |got - ref64| / scale element by element, the
    scale being the sum of the absolute terms of each output (max(1, that) behind a transcendental function), e32 the error of
    the same reference function run in fp32 on the GPU on the same inputs, never the kernel's own output.
No element is left out of any comparison: the share of excluded elements is zero (MUL_RELU_MASK takes its mask as an input, and a
RELU output near zero is small on the scale of its terms).

Output buffers are longer than needed and pre-filled with a NaN pattern no finite input produces: none may remain inside the
range, all must survive around it; outputs an epilogue does not have are passed as such buffers and must stay untouched.
Unaligned operands are slices one float into an aligned allocation.  GSVC_PRINT_ERRORS=1 prints e_kernel and e32 of every case.
"""
import ctypes as C

import pytest
import torch

from tests import _linear_kernel_refs as R
from tests._linear_kernel_refs import EPS32, PRINT, err

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF            # a quiet NaN with a payload
PAD = 8
E_INVALID, E_UNSUPPORTED = -1, -3
f64, f32 = torch.float64, torch.float32

# Bounds set by measurement for the transcendental epilogues (e_kernel on the scale max(1, A)): None = the project's rule holds for that
# output over every case of this file, so none is needed.  Measured on the MI355X, worst e_kernel / worst e32 over the file:
# TANH 1.6e-7 / 1.6e-7, SIGMOID 5.6e-8 / 4.7e-8, GELU_DUAL's Y2 2.7e-7 / 2.7e-7 (3.6e-7 / 3.6e-7 in shared_input), MUL_GELU_GRAD
# 2.6e-7 / 2.5e-7: the worst case stands at 0.30 of 4 * e32 + 4 * eps32.
TRANS_BOUND = {R.TANH: None, R.SIGMOID: None, R.GELU_DUAL: None, R.MUL_GELU_GRAD: None}


def _lib():
    from gsvc_amd import _lib
    return _lib, _lib.lib(), _lib.current_stream()


class Out:
    """n floats at an offset of `off` floats into a sentinel-filled allocation, PAD sentinels behind."""

    def __init__(self, n, off=0):
        self.n, self.off = n, off
        self.bits = torch.full((off + n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.ptr = self.bits.data_ptr() + 4 * off
        assert self.bits.data_ptr() % 16 == 0

    def fill(self, t):
        self.bits.view(f32)[self.off:self.off + self.n] = t.reshape(-1).cuda()

    def guards(self):
        return bool((self.bits[:self.off] == SENTINEL).all()) and bool((self.bits[self.off + self.n:] == SENTINEL).all())

    def written(self):
        return self.guards() and bool((self.bits[self.off:self.off + self.n] != SENTINEL).all())

    def untouched(self):
        return bool((self.bits == SENTINEL).all())

    def get(self, *shape):
        return self.bits.view(f32)[self.off:self.off + self.n].view(*shape).clone()


def _dev(t, off=0):
    """t on the GPU, `off` floats into a fresh (aligned) allocation."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 4, dtype=f32, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off
    return v


def _p(t):
    return None if t is None else t.data_ptr()


def _rule(tag, e_k, e32, bound=None):
    if PRINT:
        print(f"LINEAR_ERR {tag}: kernel {e_k:.3e} fp32 statement {e32:.3e}")
    if bound is not None:
        assert e_k <= bound, (tag, e_k, bound)
    else:
        assert e_k <= 4 * e32 + 4 * EPS32, (tag, e_k, e32)


def _exact(tag, got, ref64):
    assert torch.equal(got.double(), ref64), (tag, int((got.double() != ref64).sum()), "elements differ from the float64 result")


# ====================================================================================================== the layer kernel
def _layer(inp, M, K, N, wio, code, entry="ex", off=None, inplace=False, bias=True):
    """One call of gsvc_linear_forward (entry "plain": codes NONE / RELU) or gsvc_linear_forward_ex; returns (Y, Y2, Y3)."""
    lb, L, st = _lib()
    o = dict(x=0, y=0, aux1=0, aux2=0, y2=0, y3=0)
    o.update(off or {})
    X, W, b, a1, a2 = inp
    dX, dW, db = _dev(X, o["x"]), _dev(W), _dev(b if bias else None)
    Y, Y2, Y3 = Out(M * N, o["y"]), Out(M * N, o["y2"]), Out(M * N, o["y3"])
    if entry == "plain":
        assert code in (R.NONE, R.RELU)
        rc = L.gsvc_linear_forward(_p(dX), _p(dW), _p(db), Y.ptr, M, K, N, int(wio), int(code == R.RELU), st)
    else:
        A1 = _dev(a1, o["aux1"]) if code in R.NEEDS_AUX1 else None
        A2 = _dev(a2, o["aux2"]) if code in R.NEEDS_AUX2 else None
        p1 = _p(A1)
        if inplace:
            assert code == R.ADD
            Y.fill(a1)
            p1 = Y.ptr
        rc = L.gsvc_linear_forward_ex(_p(dX), _p(dW), _p(db), Y.ptr, M, K, N, int(wio), code, p1, _p(A2), Y2.ptr, Y3.ptr, st)
    lb.check(rc, "gsvc_linear_forward" + ("" if entry == "plain" else "_ex"))
    torch.cuda.synchronize()
    assert Y.written(), "Y"
    assert Y2.written() if (entry == "ex" and code in R.HAS_Y2) else Y2.untouched(), "Y2"
    assert Y3.written() if (entry == "ex" and code in R.HAS_Y3) else Y3.untouched(), "Y3"
    return Y.get(M, N), (Y2.get(M, N) if code in R.HAS_Y2 else None), (Y3.get(M, N) if code in R.HAS_Y3 else None)


class LayerRef:
    """v and A of one input set in float64 and fp32 on the GPU, computed once; the epilogues are applied per code."""

    def __init__(self, inp, wio, bias=True):
        self.t = {}
        for dt in (f64, f32):
            X, W, b, a1, a2 = (t.cuda().to(dt) for t in inp)
            v, A = R.linear_ref(X, W, b if bias else None, wio)
            self.t[dt] = (v, A, a1, a2)

    def outputs(self, code, dt):
        v, A, a1, a2 = self.t[dt]
        return R.epilogue_ref(code, v, a1, a2)

    def scales(self, code):
        v, A, a1, a2 = self.t[f64]
        return R.epilogue_scale(code, A, a1, a2)


def _check_layer(tag, code, got, ref, exact):
    r64, r32, sc = ref.outputs(code, f64), ref.outputs(code, f32), ref.scales(code)
    for i, name in enumerate(("Y", "Y2", "Y3")):
        if r64[i] is None:
            assert got[i] is None
            continue
        trans = (code in R.TRANSCENDENTAL) and (name == "Y2" if code == R.GELU_DUAL else True)
        if exact:
            if not trans:
                _exact(f"{tag} {name}", got[i], r64[i])
            continue
        _rule(f"{tag} {name}", err(got[i], r64[i], sc[i]), err(r32[i], r64[i], sc[i]), TRANS_BOUND[code] if trans else None)


def _single_element(tag, M, K, N, wio, code, entry):
    """X[M - 1, K - 1] = 3 and W[N - 1, K - 1] = 2 alone, no bias: Y[M - 1, N - 1] = 6 and nothing else (aux1 = 1, aux2 = 0: ADD
    lifts every element by one)."""
    inp = R.layer_inputs("one", M, K, N, wio, 0)
    y = _layer(inp, M, K, N, wio, code, entry=entry, bias=False)[0]
    want = torch.full((M, N), 1.0 if code == R.ADD else 0.0, device="cuda")
    want[M - 1, N - 1] += 6.0
    assert torch.equal(y, want), (tag, y.nonzero().tolist()[:8])


@pytest.mark.parametrize("wio", [False, True], ids=["w_nk", "w_kn"])
@pytest.mark.parametrize("K,N", R.LAYER_SHAPES)
def test_layer_shapes(K, N, wio):
    """k_linear_ws through gsvc_linear_forward (relu off and on) and gsvc_linear_forward_ex (NONE) at every listed (K, N) and row
    count: fewer rows than a 16-row block, than a wave's share, than a workgroup's; the second round of the persistent loop at
    65536 + 17 rows (16 waves) and 32768 + 17 rows (8 waves)."""
    for M in R.LAYER_M + R.LAYER_M_MORE.get((K, N), []):
        tag = f"layer K{K} N{N} M{M} {'kn' if wio else 'nk'}"
        for kind in ("int", "randn"):
            inp = R.layer_inputs(kind, M, K, N, wio, 1000 + K + N)
            ref = LayerRef(inp, wio)
            for code, entry in ((R.NONE, "plain"), (R.RELU, "plain"), (R.NONE, "ex")):
                got = _layer(inp, M, K, N, wio, code, entry=entry)
                _check_layer(f"{tag} {R.EPI_NAMES[code]}/{entry} {kind}", code, got, ref, kind == "int")
        _single_element(tag, M, K, N, wio, R.NONE, "plain")


@pytest.mark.parametrize("K,N", [(R.EPI_K, n) for n in R.EPI_N] + R.EPI_1024)
def test_layer_epilogues(K, N):
    """All ten epilogue programs on their own: one N per translation unit and store width (K = 66: the 512-thread kernels) and the
    two smallest shapes of the 1024-thread epilogue kernels.  ADD runs with a separate aux1 and in place (aux1 = Y).  The
    transcendental outputs (TANH, SIGMOID, GELU_DUAL's Y2, MUL_GELU_GRAD) are held to the same rule as the rest: measured on the
    MI355X their worst e_kernel is 1.6e-7, 5.6e-8, 2.7e-7 and 2.6e-7 against e32 of 1.6e-7, 4.7e-8, 2.7e-7 and 2.5e-7."""
    for M in R.EPI_M:
        for wio in (False, True):
            for kind in ("int", "randn"):
                inp = R.layer_inputs(kind, M, K, N, wio, 2000 + N + M)
                ref = LayerRef(inp, wio)
                for code in range(10):
                    if kind == "int" and code not in R.EXACT_EPILOGUES:
                        continue
                    tag = f"epi {R.EPI_NAMES[code]} K{K} N{N} M{M} {'kn' if wio else 'nk'} {kind}"
                    got = _layer(inp, M, K, N, wio, code)
                    _check_layer(tag, code, got, ref, kind == "int")
                    if code == R.ADD:
                        inplace = _layer(inp, M, K, N, wio, code, inplace=True)
                        assert torch.equal(inplace[0], got[0]), tag + " in place"
            for code in (R.MUL_RELU_MASK, R.FILM, R.FILM_GRAD, R.ADD):
                _single_element(f"epi {R.EPI_NAMES[code]} K{K} N{N} M{M}", M, K, N, wio, code, "ex")


@pytest.mark.parametrize("K,N", R.ALIGN_SHAPES)
def test_layer_alignment(K, N):
    """K % 4 == 0 (or K % 2 == 0) and N % 4 == 0, but X, Y, aux1 or Y2 start one float into an aligned allocation: the kernel must
    take the narrow loads (VEC 1) / stores (sv 1), and give the aligned run's bits (the width changes no summation order)."""
    M = R.ALIGN_M
    for wio in (False, True):
        for kind in ("int", "randn"):
            inp = R.layer_inputs(kind, M, K, N, wio, 3000 + K)
            ref = LayerRef(inp, wio)
            base_plain = _layer(inp, M, K, N, wio, R.NONE, entry="plain")
            _check_layer(f"align plain K{K} {kind}", R.NONE, base_plain, ref, kind == "int")
            for which in ("x", "y"):
                got = _layer(inp, M, K, N, wio, R.NONE, entry="plain", off={which: 1})
                assert torch.equal(got[0], base_plain[0]), (K, N, wio, kind, which)
            for code in (R.FILM, R.FILM_GRAD, R.GELU_DUAL, R.ADD):
                base = _layer(inp, M, K, N, wio, code)
                _check_layer(f"align {R.EPI_NAMES[code]} K{K} {kind}", code, base, ref, kind == "int")
                for which in ("x", "y", "aux1", "aux2", "y2", "y3"):
                    got = _layer(inp, M, K, N, wio, code, off={which: 1})
                    for a, b in zip(got, base):
                        assert (a is None and b is None) or torch.equal(a, b), (K, N, wio, kind, R.EPI_NAMES[code], which)


# ============================================================================================= accumulate_many / shared_input
def _accum(jobs, M, N, y_off=0):
    lb, L, st = _lib()
    arr = (lb.AccumJobC * len(jobs))()
    keep = []
    for i, (X, W) in enumerate(jobs):
        dX, dW = _dev(X), _dev(W)
        keep += [dX, dW]
        arr[i].X, arr[i].W, arr[i].K, arr[i].pad = dX.data_ptr(), dW.data_ptr(), X.shape[1], 0
    Y = Out(M * N, y_off)
    lb.check(L.gsvc_linear_accumulate_many(arr, len(jobs), Y.ptr, M, N, st), "gsvc_linear_accumulate_many")
    torch.cuda.synchronize()
    assert Y.written()
    return Y.get(M, N)


@pytest.mark.parametrize("Ks,N,M", R.ACCUM_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_accumulate_many(Ks, N, M):
    """Y = sum_p X_p W_p in one launch: 1, 2 and 8 products of mixed K_p, one block and two blocks per wave, the float4 and the
    scalar weight staging (N % 4), the three store widths (Y one float off an aligned address included)."""
    tag = f"accum Ks{Ks} N{N} M{M}"
    for kind in ("int", "randn", "one"):
        jobs = R.accum_inputs(kind, M, Ks, N, 7)
        got = _accum(jobs, M, N)
        r64, A = R.accumulate_ref([(x.cuda().double(), w.cuda().double()) for x, w in jobs])
        if kind == "randn":
            r32, _ = R.accumulate_ref([(x.cuda(), w.cuda()) for x, w in jobs])
            _rule(tag, err(got, r64, A), err(r32, r64, A))
        else:
            _exact(f"{tag} {kind}", got, r64)
            if kind == "one":
                assert got.nonzero().tolist() == [[M - 1, N - 1]]
        if M <= 4097:
            assert torch.equal(_accum(jobs, M, N, y_off=1), got), tag + " unaligned Y"


def _shared(X, jobs, wants, M, K, y_off=0):
    lb, L, st = _lib()
    arr = (lb.SharedInputJobC * len(jobs))()
    dX = _dev(X)
    keep, outs = [dX], []
    for i, ((W, b), want2) in enumerate(zip(jobs, wants)):
        N = W.shape[0]
        dW, db = _dev(W), _dev(b)
        Y, Y2 = Out(M * N, y_off), (Out(M * N, y_off) if want2 else None)
        keep += [dW, db]
        outs.append((Y, Y2, N))
        arr[i].W, arr[i].bias, arr[i].Y, arr[i].Y2, arr[i].N, arr[i].pad = dW.data_ptr(), _p(db), Y.ptr, (Y2.ptr if want2 else None), N, 0
    lb.check(L.gsvc_linear_forward_shared_input(dX.data_ptr(), M, K, arr, len(jobs), st), "gsvc_linear_forward_shared_input")
    torch.cuda.synchronize()
    res = []
    for Y, Y2, N in outs:
        assert Y.written() and (Y2 is None or Y2.written())
        res.append((Y.get(M, N), Y2.get(M, N) if Y2 is not None else None))
    return res


@pytest.mark.parametrize("K,Ns,M", R.SHARED_CASES, ids=lambda v: "-".join(f"{n}{'g' if g else ''}" for n, g in v) if isinstance(v, list) else str(v))
def test_shared_input(K, Ns, M):
    """Y_p = X W_p^T + b_p (and Y2_p = GELU(Y_p) where asked) for 1, 3 and 8 layers reading the same rows in one launch."""
    wants = [g for _, g in Ns]
    tag = f"shared K{K} Ns{[n for n, _ in Ns]} M{M}"
    for kind in ("int", "randn", "one"):
        X, jobs = R.shared_inputs(kind, M, K, [n for n, _ in Ns], 9)
        got = _shared(X, jobs, wants, M, K)
        r64 = R.shared_input_ref(X.cuda().double(), [(w.cuda().double(), b.cuda().double()) for w, b in jobs])
        r32 = R.shared_input_ref(X.cuda(), [(w.cuda(), b.cuda()) for w, b in jobs]) if kind == "randn" else None
        for p, ((y, y2), (v, g, A)) in enumerate(zip(got, r64)):
            if kind == "randn":
                _rule(f"{tag} Y{p}", err(y, v, A), err(r32[p][0], v, A))
                if y2 is not None:
                    one = A.clamp_min(1.0)
                    _rule(f"{tag} Y2_{p}", err(y2, g, one), err(r32[p][1], g, one), TRANS_BOUND[R.GELU_DUAL])
            else:
                _exact(f"{tag} {kind} Y{p}", y, v)
                if kind == "one":
                    assert y.nonzero().tolist() == [[M - 1, y.shape[1] - 1]]
        if kind == "randn" and M <= 4097:
            for (a, a2), (b, b2) in zip(_shared(X, jobs, wants, M, K, y_off=1), got):
                assert torch.equal(a, b) and (a2 is None or torch.equal(a2, b2)), tag + " unaligned Y"


# ====================================================================================================== weight gradients
def _per_slot(N, K, want_db):
    return N * K + (N if want_db else 0)


def _wgrad(G, X, want_db, ws_floats, g_off=0, x_off=0):
    """One gsvc_linear_wgrad call; returns (dW, db or None)."""
    lb, L, st = _lib()
    (M, N), K = G.shape, X.shape[1]
    dG, dX = _dev(G, g_off), _dev(X, x_off)
    dW, db, ws = Out(N * K), Out(N), Out(ws_floats)
    lb.check(L.gsvc_linear_wgrad(dG.data_ptr(), dX.data_ptr(), dW.ptr, db.ptr if want_db else None, M, N, K, ws.ptr, ws_floats, st),
             "gsvc_linear_wgrad")
    torch.cuda.synchronize()
    assert dW.written() and (db.written() if want_db else db.untouched()) and ws.guards()
    return dW.get(N, K), (db.get(N) if want_db else None)


_wgrad_ref_cache = {}


def _wgrad_refs(G, X):
    """(float64 reference with its scales, fp32 statement) of one input pair on the GPU, computed once."""
    key = (id(G), id(X))
    if key not in _wgrad_ref_cache:
        _wgrad_ref_cache.clear()
        _wgrad_ref_cache[key] = (G, X, R.wgrad_ref(G.cuda().double(), X.cuda().double()), R.wgrad_ref(G.cuda(), X.cuda()))
    return _wgrad_ref_cache[key][2:]


def _check_wgrad(tag, got, G, X, exact):
    dW, db = got
    r, r32 = _wgrad_refs(G, X)
    if exact:
        _exact(tag + " dW", dW, r[0])
        if db is not None:
            _exact(tag + " db", db, r[1])
        return
    _rule(tag + " dW", err(dW, r[0], r[2]), err(r32[0], r[0], r[2]))
    if db is not None:
        _rule(tag + " db", err(db, r[1], r[3]), err(r32[1], r[1], r[3]))


@pytest.mark.parametrize("N,K", R.WGRAD_SHAPES)
def test_wgrad_shapes(N, K):
    """gsvc_linear_wgrad at every listed (N, K) and row count, db wanted and NULL; at 17 and 4097 rows with a workspace of exactly
    1 slot, 3 slots, gsvc_linear_wgrad_workspace() and twice that; two calls give the same bits (no atomics)."""
    lb, L, st = _lib()
    full = int(L.gsvc_linear_wgrad_workspace(N, K))
    assert full == 256 * (N * K + N)
    for M in R.WGRAD_M:
        for kind in ("int", "randn", "one"):
            G, X = R.wgrad_inputs(kind, M, N, K, 100 + N + K)
            for want_db in (True, False):
                ps = _per_slot(N, K, want_db)
                sizes = [ps, 3 * ps, full, 2 * full] if (M in (17, 4097) and kind != "one") else [full]
                for ws in sizes:
                    tag = f"wgrad N{N} K{K} M{M} db{int(want_db)} ws{ws // ps} {kind}"
                    got = _wgrad(G, X, want_db, ws)
                    _check_wgrad(tag, got, G, X, kind != "randn")
                    if kind == "one":
                        assert got[0].nonzero().tolist() == [[N - 1, K - 1]] and (got[1] is None or got[1].nonzero().tolist() == [[N - 1]])
                    if kind == "randn" and ws == full:
                        again = _wgrad(G, X, want_db, ws)
                        assert torch.equal(again[0], got[0]) and (got[1] is None or torch.equal(again[1], got[1])), tag + " twice"


@pytest.mark.parametrize("N,K", R.WGRAD_BIG_SHAPES)
def test_wgrad_many_rows(N, K):
    """70001 rows: every slot of the workspace in use and several chunks per row split.  The exact probe draws G from {-1, 0, 1}."""
    M = R.WGRAD_M_BIG
    full = 256 * (N * K + N)
    G, X = R.wgrad_inputs("int", M, N, K, 100 + N + K, g_bound=1)
    _check_wgrad(f"wgrad N{N} K{K} M{M} int", _wgrad(G, X, True, full), G, X, True)
    G, X = R.wgrad_inputs("randn", M, N, K, 100 + N + K)
    for want_db in (True, False):
        _check_wgrad(f"wgrad N{N} K{K} M{M} db{int(want_db)} randn", _wgrad(G, X, want_db, full), G, X, False)


def test_wgrad_alignment():
    """G and X of (100, 100) one float into an aligned allocation: other tile splits (3 tiles a block instead of 4), the same
    product under the float64 rule."""
    N = K = 100
    full = 256 * (N * K + N)
    for M in (17, 4097):
        for g_off, x_off in ((1, 0), (0, 1), (1, 1)):
            for kind in ("int", "randn"):
                G, X = R.wgrad_inputs(kind, M, N, K, 5)
                _check_wgrad(f"wgrad unaligned G{g_off} X{x_off} M{M} {kind}", _wgrad(G, X, True, full, g_off, x_off), G, X, kind == "int")


# (N, K, M, want_db, workspace slots): thirteen products that fit a batch launch first (the batch flushes at 12 and starts a
# second launch), then (192, 192) (9 wave pairs: 12 % 9 != 0) and (177, 177) (launch_wgrad2), which go alone, between two more
# batch products; every M differs; job 4 has a workspace of a single slot, job 9 of three.
BATCH_JOBS = [(100, 100, 4097, 1, 256), (23, 17, 1, 1, 256), (66, 66, 17, 0, 256), (100, 50, 257, 1, 256), (129, 33, 1000, 1, 1),
              (49, 81, 33, 0, 256), (82, 130, 2049, 1, 256), (10, 100, 15, 1, 256), (1, 50, 16, 0, 256), (30, 100, 513, 1, 3),
              (70, 100, 77, 1, 256), (100, 116, 64, 0, 256), (100, 100, 100, 1, 512),
              (192, 192, 301, 1, 256), (66, 66, 129, 1, 256), (177, 177, 263, 0, 256), (23, 17, 4001, 1, 256)]


@pytest.mark.parametrize("kind", ["int", "randn"])
def test_wgrad_batch(kind):
    """gsvc_linear_wgrad_partial_many over 17 products in one call and gsvc_linear_wgrad_reduce_many over the 17 (more than the 16
    of one reduce launch): each product's dW / db under the float64 rule (bit for bit on the integer probe) and as close to its own
    gsvc_linear_wgrad result; slots_used within [1, min(256, workspace slots)]; the sentinels between the workspace regions
    survive: no product writes into another's region."""
    lb, L, st = _lib()
    n = len(BATCH_JOBS)
    assert n == 17
    GAP = 64
    sizes = [slots * _per_slot(N, K, db) for N, K, M, db, slots in BATCH_JOBS]
    starts, at = [], GAP
    for s in sizes:
        starts.append(at)
        at += (s + 3) // 4 * 4 + GAP          # regions start 16-byte aligned
    arena = torch.full((at,), SENTINEL, dtype=torch.int32, device="cuda")
    pj, rj = (lb.WgradPartialJobC * n)(), (lb.WgradReduceJobC * n)()
    data, outs = [], []
    for i, (N, K, M, db, slots) in enumerate(BATCH_JOBS):
        G, X = R.wgrad_inputs(kind, M, N, K, 40 + i)
        dG, dX = _dev(G), _dev(X)
        data.append((G, X, dG, dX))
        pj[i].G, pj[i].X, pj[i].workspace = dG.data_ptr(), dX.data_ptr(), arena.data_ptr() + 4 * starts[i]
        pj[i].M, pj[i].workspace_floats, pj[i].want_db, pj[i].N, pj[i].K, pj[i].slots_used = M, sizes[i], db, N, K, -1
    lb.check(L.gsvc_linear_wgrad_partial_many(pj, n, st), "gsvc_linear_wgrad_partial_many")
    torch.cuda.synchronize()
    for i, (N, K, M, db, slots) in enumerate(BATCH_JOBS):
        used = pj[i].slots_used
        assert 1 <= used <= min(256, slots), (i, used)
        region = arena[starts[i]:starts[i] + sizes[i]]
        ps = _per_slot(N, K, db)
        assert bool((region[:used * ps] != SENTINEL).all()) and bool((region[used * ps:] == SENTINEL).all()), i
        dW, dbo = Out(N * K), Out(N)
        outs.append((dW, dbo))
        rj[i].partial, rj[i].dW, rj[i].db = arena.data_ptr() + 4 * starts[i], dW.ptr, (dbo.ptr if db else None)
        rj[i].slots, rj[i].N, rj[i].K = used, N, K
    # everything between and around the regions
    mask = torch.ones(at, dtype=torch.bool, device="cuda")
    for s, z in zip(starts, sizes):
        mask[s:s + z] = False
    assert bool((arena[mask] == SENTINEL).all()), "a product wrote outside its workspace region"
    lb.check(L.gsvc_linear_wgrad_reduce_many(rj, n, st), "gsvc_linear_wgrad_reduce_many")
    torch.cuda.synchronize()
    for i, (N, K, M, db, slots) in enumerate(BATCH_JOBS):
        G, X = data[i][:2]
        dW, dbo = outs[i]
        assert dW.written() and (dbo.written() if db else dbo.untouched()), i
        got = (dW.get(N, K), dbo.get(N) if db else None)
        tag = f"wgrad batch job{i} N{N} K{K} M{M} {kind}"
        _check_wgrad(tag, got, G, X, kind == "int")
        single = _wgrad(G, X, bool(db), 256 * _per_slot(N, K, db))
        if kind == "int":
            assert torch.equal(single[0], got[0]) and (not db or torch.equal(single[1], got[1])), tag
        else:
            r, r32 = _wgrad_refs(G, X)
            _rule(tag + " dW against the single call", err(got[0], single[0], r[2]), err(r32[0], r[0], r[2]))
            if db:
                _rule(tag + " db against the single call", err(got[1], single[1], r[3]), err(r32[1], r[1], r[3]))


# ====================================================================================================== refusals and M = 0
def test_layer_refusals_leave_outputs_untouched():
    """Unsupported widths, an unknown epilogue and an epilogue without its operand: the error code, nothing written."""
    lb, L, st = _lib()
    M = 17
    X, a1, a2 = (_dev(torch.zeros(M * 193)) for _ in range(3))
    W, b = _dev(torch.zeros(193 * 193)), _dev(torch.zeros(193))
    for K, N in ((193, 16), (16, 193), (193, 193)):
        Y, Y2, Y3 = Out(M * N), Out(M * N), Out(M * N)
        assert L.gsvc_linear_forward(_p(X), _p(W), _p(b), Y.ptr, M, K, N, 0, 0, st) == E_UNSUPPORTED
        assert L.gsvc_linear_forward_ex(_p(X), _p(W), _p(b), Y.ptr, M, K, N, 0, R.FILM, _p(a1), _p(a2), Y2.ptr, Y3.ptr, st) == E_UNSUPPORTED
        torch.cuda.synchronize()
        assert Y.untouched() and Y2.untouched() and Y3.untouched()
    K = N = 16
    Y, Y2, Y3 = Out(M * N), Out(M * N), Out(M * N)
    calls = [(10, _p(a1), _p(a2), Y2.ptr, Y3.ptr), (-1, _p(a1), _p(a2), Y2.ptr, Y3.ptr),
             (R.MUL_GELU_GRAD, None, _p(a2), Y2.ptr, Y3.ptr), (R.FILM, _p(a1), None, Y2.ptr, Y3.ptr),
             (R.FILM, _p(a1), _p(a2), None, Y3.ptr), (R.FILM_GRAD, _p(a1), _p(a2), Y2.ptr, None),
             (R.GELU_DUAL, None, None, None, None), (R.ADD, None, None, None, None)]
    for code, p1, p2, q2, q3 in calls:
        assert L.gsvc_linear_forward_ex(_p(X), _p(W), _p(b), Y.ptr, M, K, N, 0, code, p1, p2, q2, q3, st) == E_INVALID, code
        assert b"linear_forward_ex" in L.gsvc_last_error()
    torch.cuda.synchronize()
    assert Y.untouched() and Y2.untouched() and Y3.untouched()
    # M = 0: nothing to do, nothing written
    assert L.gsvc_linear_forward(_p(X), _p(W), _p(b), Y.ptr, 0, K, N, 0, 1, st) == 0
    assert L.gsvc_linear_forward_ex(_p(X), _p(W), _p(b), Y.ptr, 0, K, N, 0, R.FILM_GRAD, _p(a1), _p(a2), Y2.ptr, Y3.ptr, st) == 0
    torch.cuda.synchronize()
    assert Y.untouched() and Y2.untouched() and Y3.untouched()


def test_many_refusals_leave_outputs_untouched():
    lb, L, st = _lib()
    X = _dev(torch.zeros(65537 * 4))
    W = _dev(torch.zeros(193 * 193))
    Y = Out(65537 * 2)

    def accum(n, K, N, M):
        arr = (lb.AccumJobC * n)()
        for i in range(n):
            arr[i].X, arr[i].W, arr[i].K = X.data_ptr(), W.data_ptr(), K
        return L.gsvc_linear_accumulate_many(arr, n, Y.ptr, M, N, st)

    def shared(n, K, N, M):
        arr = (lb.SharedInputJobC * n)()
        for i in range(n):
            arr[i].W, arr[i].bias, arr[i].Y, arr[i].Y2, arr[i].N = W.data_ptr(), None, Y.ptr, Y.ptr, N
        return L.gsvc_linear_forward_shared_input(X.data_ptr(), M, K, arr, n, st)

    assert accum(9, 2, 1, 17) == E_UNSUPPORTED           # nine products
    assert accum(2, 51, 1, 17) == E_UNSUPPORTED          # an odd K_p
    assert accum(1, 2, 1, 65537) == E_UNSUPPORTED        # more rows than two blocks per wave cover
    assert accum(1, 2, 193, 17) == E_UNSUPPORTED and accum(1, 193, 2, 17) == E_UNSUPPORTED and accum(1, 194, 2, 17) == E_UNSUPPORTED
    assert shared(9, 4, 1, 17) == E_UNSUPPORTED
    assert shared(1, 50, 1, 17) == E_UNSUPPORTED         # K not a multiple of 4
    assert shared(1, 4, 161, 17) == E_UNSUPPORTED
    assert shared(1, 4, 1, 65537) == E_UNSUPPORTED
    assert shared(1, 193, 1, 17) == E_UNSUPPORTED and shared(1, 196, 1, 17) == E_UNSUPPORTED and shared(1, 4, 193, 17) == E_UNSUPPORTED
    assert accum(1, 2, 1, 0) == 0 and shared(1, 4, 1, 0) == 0      # M = 0: a no-op
    torch.cuda.synchronize()
    assert Y.untouched()


def test_wgrad_refusals_and_no_rows():
    lb, L, st = _lib()
    M = 17
    G, X = _dev(torch.zeros(M * 193)), _dev(torch.zeros(M * 193))
    for N, K in ((193, 16), (16, 193)):
        dW, db, ws = Out(N * K), Out(N), Out(4 * (N * K + N))
        used = C.c_int32(-7)
        assert L.gsvc_linear_wgrad(_p(G), _p(X), dW.ptr, db.ptr, M, N, K, ws.ptr, ws.n, st) == E_UNSUPPORTED
        assert L.gsvc_linear_wgrad_partial(_p(G), _p(X), 1, M, N, K, ws.ptr, ws.n, C.byref(used), st) == E_UNSUPPORTED
        pj = (lb.WgradPartialJobC * 1)()
        pj[0].G, pj[0].X, pj[0].workspace, pj[0].M, pj[0].workspace_floats = _p(G), _p(X), ws.ptr, M, ws.n
        pj[0].want_db, pj[0].N, pj[0].K = 1, N, K
        assert L.gsvc_linear_wgrad_partial_many(pj, 1, st) == E_UNSUPPORTED
        # the reduce refuses as a whole, the supported jobs in front of the unsupported one included
        rj = (lb.WgradReduceJobC * 18)()
        for i in range(18):
            bad = i == 17
            rj[i].partial, rj[i].dW, rj[i].db, rj[i].slots = ws.ptr, dW.ptr, db.ptr, 1
            rj[i].N, rj[i].K = (N, K) if bad else (1, 1)
        assert L.gsvc_linear_wgrad_reduce_many(rj, 18, st) == E_UNSUPPORTED
        torch.cuda.synchronize()
        assert dW.untouched() and db.untouched() and ws.untouched() and used.value == -7
    # a workspace one float short of a slot, with and without db
    N, K = 23, 17
    for want_db in (True, False):
        ps = _per_slot(N, K, want_db)
        dW, db, ws = Out(N * K), Out(N), Out(ps)
        assert L.gsvc_linear_wgrad(_p(G), _p(X), dW.ptr, db.ptr if want_db else None, M, N, K, ws.ptr, ps - 1, st) == E_INVALID
        used = C.c_int32(-7)
        assert L.gsvc_linear_wgrad_partial(_p(G), _p(X), int(want_db), M, N, K, ws.ptr, ps - 1, C.byref(used), st) == E_INVALID
        torch.cuda.synchronize()
        assert dW.untouched() and db.untouched() and ws.untouched() and used.value == -7
    # M = 0: the gradients of no rows are zero
    dW, db, ws = Out(N * K), Out(N), Out(N * K + N)
    assert L.gsvc_linear_wgrad(None, None, dW.ptr, db.ptr, 0, N, K, ws.ptr, ws.n, st) == 0
    torch.cuda.synchronize()
    assert dW.written() and db.written() and ws.untouched()
    assert not dW.get(N * K).any() and not db.get(N).any()
