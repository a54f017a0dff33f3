"""The hash-grid kernels of csrc/grid.hip called through their C entry points on raw buffers: gsvc_grid_forward / _backward, the
strided _ex forms, the multi-grid _many forms, gsvc_pack_sign_bits and gsvc_grid_forward_packed, each against the float64 run of the
plain tensor statement in tests/_grid_kernel_refs.py (pinned without a GPU by tests/test_grid_kernel_refs_cpu.py).

Error rule: e_kernel <= 4 * e32 + 4 * eps32, both errors against the float64 statement, e32 being the error of the same statement
run in fp32 on the GPU on the same inputs (for the table gradient: index_add_ of the fp32 contributions), never the kernel's own
output.  Scales: features on max|table| of the level, dy_dx on (res - 2) * max|table| of the level, the table gradient on max|ref|
of each (level, channel) block, the input gradient on max|ref|.  Exact compares wherever the result is one table row, an exact
mean, an exact fixed-point sum or must be zero / untouched.  Output buffers are allocated PAD elements longer than needed and
pre-filled with a NaN pattern no finite input produces: none may remain inside the written range, all must survive past it.
Every pointer handed over is 16-byte aligned and every level starts on a multiple of 8 rows (the library does not refuse misaligned
feature blocks; they are not passed).  GSVC_PRINT_ERRORS=1 prints e_kernel and e32 of every case.

Which path of k_grid_bwd_lds a case takes, from the kernel's conditions (LDS: at most 16 slices of 147456 / (8 * (C + 1)) rows,
at most 65536 rows, level maximum finite and >= 2^-60; else global float atomics):
  (a) all LDS.  (c) 1000 rows, 65536 rows with C = 1 (4 slices) and C = 2 (11 slices): LDS; 65536 rows with C = 4 (18 slices) and
  65544 rows: fallback.  (d) SLICE_ROWS + 8 rows (2 slices), 32768 rows at C = 8 and 8928 rows at C = 32 (16 slices): LDS; 32776 and
  8936 rows (17 slices): fallback.  (e) LDS.  (f) LDS except the level of magnitude 1e-25 (float path).  (g) LDS.  (h) LDS except
  the levels of magnitude 1e-25.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests._grid_kernel_refs import (EPS32, PRINT, GridIO, err, grid_backward_ref, grid_case, grid_forward_ref, grid_rows,
                                     io_default, io_extract, io_place, io_points)

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF            # a quiet NaN with a payload
PAD = 8


def _sentinel(n):
    return torch.full((n + PAD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _written(buf, n):
    """Every element of [0, n) was written, none past n."""
    bits = buf.view(torch.int32)
    return bool((bits[:n] != SENTINEL).all()) and bool((bits[n:] == SENTINEL).all())


def _untouched(buf):
    return bool((buf.view(torch.int32) == SENTINEL).all())


def _zeros_guarded(n):
    """n zeros followed by the sentinel (for buffers the kernel adds to)."""
    b = _sentinel(n)
    b[:n] = 0
    return b


def _tail_kept(buf, n):
    return bool((buf.view(torch.int32)[n:] == SENTINEL).all())


def _lib():
    from gsvc_amd import _lib
    return _lib, _lib.lib(), _lib.current_stream()


def _p(t):
    """Device pointer of a tensor (None -> NULL); 16-byte aligned or the test is wrong."""
    from gsvc_amd import _lib
    if t is None:
        return None
    assert t.data_ptr() % 16 == 0 and t.is_contiguous()
    return _lib.ptr(t)


def _rule(tag, e_k, e32):
    if PRINT:
        print(f"GRID_ERR {tag}: kernel {e_k:.3e} fp32 statement {e32:.3e}")
    assert e_k <= 4 * e32 + 4 * EPS32, (tag, e_k, e32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _i32dev(v):
    return torch.tensor([int(o) for o in v], dtype=torch.int32, device="cuda")


def _levels(D, res, log2):
    from gsvc_amd.encodings import level_offsets
    return [int(o) for o in level_offsets(res, D, log2)]


def _ioc(io):
    from gsvc_amd import _lib
    c = _lib.GridIOC()
    c.feat_level_stride, c.feat_point_stride, c.in_stride = io.feat_level_stride, io.feat_point_stride, io.in_stride
    for k in range(3):
        c.in_col[k] = io.in_col[k] if k < len(io.in_col) else 0
    return c


# ---------------------------------------------------------------------------------------------------------------- references
class Refs:
    """The float64 and the fp32 run of the statement on the same device inputs (computed once per case)."""

    def __init__(self, x, table, off, res, grad=None, prior=None):
        self.off, self.res, self.C, self.L = off, res, table.shape[1], len(res)
        assert all(o % 8 == 0 for o in off[:-1])            # every level starts on a multiple of 8 rows
        self.out64, self.dy64, self.loc64 = grid_forward_ref(x, table, off, res, torch.float64)
        self.out32, self.dy32, self.loc32 = grid_forward_ref(x, table, off, res, torch.float32)
        tmax = torch.stack([table[off[l]:off[l + 1]].abs().max() for l in range(self.L)]).double()
        self.s_out = tmax.view(self.L, 1, 1)
        self.s_dy = (tmax * (torch.tensor(res, device="cuda").double() - 2)).view(1, self.L, 1, 1)
        self.outside = ((x < 0) | (x > 1)).any(dim=1)
        if grad is not None:
            self.table_grad(grad, prior)

    def table_grad(self, grad, prior=None):
        """gt64 / gt32: prior + gradient in either precision; s_gt: max|gradient| of each (level, channel) block; counts per row."""
        off, Cc = self.off, self.C
        pr = None if prior is None else prior[:off[-1]]
        g64, self.counts, _ = grid_backward_ref(grad, self.loc64, off, Cc, None, torch.float64)
        self.gt32, _, _ = grid_backward_ref(grad, self.loc32, off, Cc, None, torch.float32, prior=pr)
        self.gt64 = g64 if pr is None else g64 + pr.double()
        self.s_gt = torch.zeros_like(g64)
        for l in range(self.L):
            if off[l + 1] > off[l]:
                self.s_gt[off[l]:off[l + 1]] = g64[off[l]:off[l + 1]].abs().max(dim=0, keepdim=True).values
        return self

    def check_forward(self, tag, out, dy=None):
        _rule(f"{tag} out", err(out, self.out64, self.s_out), err(self.out32, self.out64, self.s_out))
        assert not out[:, self.outside].any()
        if dy is not None:
            _rule(f"{tag} dy_dx", err(dy, self.dy64, self.s_dy), err(self.dy32, self.dy64, self.s_dy))
            assert not dy[self.outside].any()

    def check_table_grad(self, tag, got, prior=None):
        """``got`` [>= off[-1], C]: the rule on each block's scale from off[0] on; rows no corner reaches keep their bits."""
        off = self.off
        lo, hi = off[0], off[-1]
        _rule(f"{tag} table gradient", err(got[lo:hi], self.gt64[lo:hi], self.s_gt[lo:hi]), err(self.gt32[lo:hi], self.gt64[lo:hi], self.s_gt[lo:hi]))
        idle = self.counts[lo:hi] == 0
        want = torch.zeros_like(got[lo:hi]) if prior is None else prior[lo:hi]
        assert torch.equal(got[lo:hi][idle].view(torch.int32), want[idle].view(torch.int32))


def _forward(x, table, off_d, res_d, N, D, Cc, L, want_dy=True):
    lb, Lh, st = _lib()
    out = _sentinel(L * N * Cc)
    dy = _sentinel(N * L * D * Cc) if want_dy else None
    lb.check(Lh.gsvc_grid_forward(_p(x), _p(table), _p(off_d), _p(res_d), _p(out), N, D, Cc, L, _p(dy), st), "gsvc_grid_forward")
    assert _written(out, L * N * Cc) and (dy is None or _written(dy, N * L * D * Cc))
    return out[:L * N * Cc].view(L, N, Cc), (dy[:N * L * D * Cc].view(N, L, D, Cc) if want_dy else None)


def _backward(grad, x, table, off_d, res_d, ge, N, D, Cc, L, dy=None):
    """ge: the guarded table-gradient buffer (accumulated into).  Returns grad_inputs [N, D] when dy_dx is given."""
    lb, Lh, st = _lib()
    gi = _sentinel(N * D) if dy is not None else None
    lb.check(Lh.gsvc_grid_backward(_p(grad), _p(x), _p(table), _p(off_d), _p(res_d), _p(ge), N, D, Cc, L, _p(dy), _p(gi), st), "gsvc_grid_backward")
    if gi is None:
        return None
    assert _written(gi, N * D)
    return gi[:N * D].view(N, D)


# ---------------------------------------------------------------------------------------------------------------- (a) forward
A_SHAPES = [(1, 1, (16, 64), 5), (2, 2, (10, 18), 8), (3, 4, (6, 9, 14), 9), (3, 8, (18, 24, 33, 44), 13), (2, 8, (130, 258), 15),
            (3, 16, (18, 40), 11), (2, 32, (20,), 7),
            (2, 2, (2, 10), 8)]          # a level of resolution 2: every corner on the border, the weight sum is zero


@pytest.mark.parametrize("D,Cc,res,log2", A_SHAPES)
def test_forward_dy_dx_and_input_gradient(D, Cc, res, log2):
    """N in {1, 255, 256, 257, 3000}: gsvc_grid_forward with dy_dx, again without (the same bits), gsvc_grid_backward with the
    kernel's own dy_dx: grad_inputs overwritten (pre-filled with the NaN pattern) and, as a function of (grad, dy_dx), by the rule
    against the float64 sum; the table gradient of the same call by the rule.  Rows outside [0, 1]^D: exactly zero everywhere.
    measured on the MI355X, largest over shapes and sizes, kernel / fp32 statement: out 1.4e-7 / 1.4e-7, dy_dx 1.9e-7 / 1.9e-7,
    table gradient 2.5e-7 / 1.2e-7, grad_inputs 4.7e-8 / 5.0e-8.  With the sum of k_grid_input_bwd formed in float, one point
    (N = 1, 4 levels of 8 features, 32 terms that cancel) gave 9.1e-7 / 8.2e-8 and missed the rule; the kernel now adds in double."""
    off = _levels(D, res, log2)
    L, rows = len(res), off[-1]
    off_d, res_d = _i32dev(off), _i32dev(res)
    for N in (1, 255, 256, 257, 3000):
        x, table, grad = (_dev(a) for a in grid_case(D, Cc, off, res, N, 1000 * D + 10 * Cc + N))
        tag = f"a D={D} C={Cc} res={res} N={N}"
        out, dy = _forward(x, table, off_d, res_d, N, D, Cc, L)
        out2, _ = _forward(x, table, off_d, res_d, N, D, Cc, L, want_dy=False)
        assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
        r = Refs(x, table, off, res, grad)
        r.check_forward(tag, out, dy)
        for l, rs in enumerate(res):
            if rs == 2:
                assert not out[l].any() and not dy[:, l].any()
        ge = _zeros_guarded(rows * Cc)
        gi = _backward(grad, x, table, off_d, res_d, ge, N, D, Cc, L, dy=dy)
        assert _tail_kept(ge, rows * Cc)
        r.check_table_grad(tag, ge[:rows * Cc].view(rows, Cc))
        _, _, gi64 = grid_backward_ref(grad, [], off, Cc, dy, torch.float64)
        _, _, gi32 = grid_backward_ref(grad, [], off, Cc, dy, torch.float32)
        sc = float(gi64.abs().max())
        if sc > 0:
            _rule(f"{tag} grad_inputs", err(gi, gi64, sc), err(gi32, gi64, sc))
        else:
            assert not gi.any()
        assert not gi[r.outside].any() and int(r.outside.sum()) == min(max(N - 2, 0), 2)


# ---------------------------------------------------------------------------------------------------------------- (b) exact
@pytest.mark.parametrize("D,Cc,res,log2", [(2, 1, (18, 34, 130, 258, 1026), 15), (2, 8, (18, 258), 12), (3, 2, (18, 34, 130), 13),
                                            (3, 8, (18, 34), 13)])
def test_exact_lookups(D, Cc, res, log2):
    """Resolutions with res - 2 a power of two.  x = (k + 0.5) / (res - 2) puts a point on the grid node k + 1 of that level
    (pos = k + 1 exactly, frac = 0): the level's feature is the table row the statement's index names, bit for bit - any wrong hash,
    stride, offset or channel fails.  x = k / (res - 2) puts it at the centre of a cell (every frac = 0.5): with a table of small
    integers the feature is the exact mean of the 2^D rows.  Dense levels (18^2, 34^2, 130^2, 18^3) and hashed ones."""
    off = _levels(D, res, log2)
    L, n = len(res), 600
    off_d, res_d = _i32dev(off), _i32dev(res)
    rng = np.random.default_rng(D * 10 + Cc)
    table = _dev(rng.standard_normal((off[-1], Cc)).astype(np.float32))
    itable = _dev(rng.integers(-8, 9, (off[-1], Cc)).astype(np.float32))
    for l, rs in enumerate(res):
        s = rs - 2
        assert s & (s - 1) == 0
        dense = rs ** D <= off[l + 1] - off[l]
        k = rng.integers(0, s, (n, D))                       # nodes 1 .. res - 2
        x = _dev(((k + 0.5) / s).astype(np.float32))
        out, _ = _forward(x, table, off_d, res_d, n, D, Cc, L, want_dy=False)
        _, _, loc = grid_forward_ref(x, table, off, res, torch.float64)
        assert bool((loc[l]["w"][:, 0] == 1).all()) and bool((loc[l]["w"][:, 1:] == 0).all()) and bool(loc[l]["valid"][:, 0].all())
        rows0 = loc[l]["rows"][:, 0]
        assert torch.equal(rows0, grid_rows(_dev(k + 1), rs, off[l + 1] - off[l]))
        if dense:
            assert torch.equal(rows0.cpu(), torch.from_numpy(sum((k[:, d] + 1) * rs ** d for d in range(D))))
        assert torch.equal(out[l].view(torch.int32), table[off[l] + rows0].view(torch.int32)), (l, rs)
        k = rng.integers(1, s, (n, D))                       # cells 1 .. res - 3: all 2^D corners interior
        x = _dev((k / s).astype(np.float32))
        out, _ = _forward(x, itable, off_d, res_d, n, D, Cc, L, want_dy=False)
        _, _, loc = grid_forward_ref(x, itable, off, res, torch.float64)
        assert bool(loc[l]["valid"].all()) and bool((loc[l]["w"] == 0.5 ** D).all())
        want = itable.double()[off[l] + loc[l]["rows"]].mean(dim=1)
        assert torch.equal(out[l].double(), want), (l, rs)


# ---------------------------------------------------------------------------------------------------------------- (c), (d) tables
def _node_point(res, node, D):
    """A float32 point inside the cell whose corner 0 is the grid node ``node``."""
    return [(float(c) - 0.5 + 0.3) / (res - 2) for c in node[:D]]


def _table_case(tag, D, Cc, res, off, N, seed, tail_rows=8):
    """Forward and backward on a table of off[-1] + tail_rows rows whose levels are off[0] .. off[-1] (written by hand): forward and
    dy_dx by the rule; the backward ACCUMULATES onto a non-zero prior: prior + gradient by the rule on each block's scale, the rows
    before off[0] and after off[-1], and every row of the levels that no corner reaches, keep the prior's bits.  Two points are
    placed on the interior nodes of level 0 with the highest and the lowest row number."""
    L, total = len(res), off[-1] + tail_rows
    x, table, grad = grid_case(D, Cc, [total], res, N, seed)
    x, table, grad = _dev(x), _dev(table), _dev(grad)
    rows0 = off[1] - off[0]
    r = torch.arange(1, res[0] - 1, device="cuda")
    nodes = torch.cartesian_prod(*([r] * D)).view(-1, D)
    nr = grid_rows(nodes, res[0], rows0)
    hi_row, lo_row = int(nr.max()), int(nr.min())
    x[9] = torch.tensor(_node_point(res[0], nodes[int(nr.argmax())].tolist(), D), device="cuda")
    x[10] = torch.tensor(_node_point(res[0], nodes[int(nr.argmin())].tolist(), D), device="cuda")
    off_d, res_d = _i32dev(off), _i32dev(res)
    out, dy = _forward(x, table, off_d, res_d, N, D, Cc, L)
    prior = (((torch.arange(total * Cc, device="cuda") % 5).float() + 1) / 4 * (1 - 2 * (torch.arange(total * Cc, device="cuda") % 2).float())).view(total, Cc)
    ref = Refs(x, table, off, res, grad, prior)
    ref.check_forward(tag, out, dy)
    assert int(ref.loc64[0]["rows"][9, 0]) == hi_row and int(ref.loc64[0]["rows"][10, 0]) == lo_row
    assert ref.counts[off[0] + hi_row] > 0 and ref.counts[off[0] + lo_row] > 0
    ge = _sentinel(total * Cc)
    ge[:total * Cc] = prior.view(-1)
    _backward(grad, x, table, off_d, res_d, ge, N, D, Cc, L)
    assert _tail_kept(ge, total * Cc)
    got = ge[:total * Cc].view(total, Cc)
    assert torch.equal(got[:off[0]], prior[:off[0]]) and torch.equal(got[off[-1]:], prior[off[-1]:])
    ref.check_table_grad(tag, got, prior)
    assert bool((got[off[0]:off[-1]][ref.counts[off[0]:] > 0] != prior[off[0]:off[-1]][ref.counts[off[0]:] > 0]).any())
    return hi_row


@pytest.mark.parametrize("D,Cc,res,off,top", [
    (3, 2, (40, 57), [0, 1000, 2000], 999),              # hashed, not a power of two: index % rows
    (2, 1, (258,), [0, 65536], 65535),                   # the largest table the 16-bit row packing holds: 4 slices
    (2, 2, (258,), [0, 65536], 65535),                   # 11 slices
    (2, 4, (258,), [0, 65536], 65535),                   # 18 slices: global atomics
    (2, 2, (258,), [0, 65544], None),                    # more than 65536 rows: global atomics, index % rows
    (2, 2, (258, 130), [8, 65544, 82448], 65535),        # the same 65536 rows away from the table's start, a dense level behind
])
def test_table_indexing_edges(D, Cc, res, off, top):
    """(c) forward and backward; the point on the highest interior node row reaches row rows - 1 where ``top`` says so (row 65535 of
    65536: all sixteen bits of a packed row index set)."""
    hi = _table_case(f"c D={D} C={Cc} res={res} off={off}", D, Cc, res, off, 6200, 31 * Cc + len(off))
    assert top is None or hi == top


SLICE_ROWS = {1: 18432, 2: 6144, 4: 3686, 8: 2048, 16: 1084, 32: 558}


@pytest.mark.parametrize("Cc,rows", [(c, r + 8) for c, r in SLICE_ROWS.items()] + [(8, 32768), (8, 32776), (32, 8928), (32, 8936)])
def test_slice_boundaries_of_the_lds_backward(Cc, rows):
    """(d) one hashed 3-D level (resolution 40) of SLICE_ROWS + 8 rows: the second slice holds 8 rows; at C = 8 and C = 32 exactly 16
    slices (LDS) and 8 rows more (17 slices: global atomics).  The level sits at rows 8 .. 8 + rows of a longer table."""
    assert all(147456 // (8 * (c + 1 if c > 1 else 1)) == r for c, r in SLICE_ROWS.items())
    assert 40 ** 3 > rows                                  # (the level starts at row 8; only a level's first row needs the 8-row alignment)
    hi = _table_case(f"d C={Cc} rows={rows}", 3, Cc, (40,), [8, 8 + rows], 6200, rows + Cc)
    sr = SLICE_ROWS[Cc]
    if (rows + sr - 1) // sr <= 16:
        assert hi >= (rows - 1) // sr * sr                 # a point reaches the last slice


# ---------------------------------------------------------------------------------------------------------------- (e) chunks
def _table_grad(grad, x, off_d, res_d, rows, N, D, Cc, L, table=None):
    ge = _zeros_guarded(rows * Cc)
    _backward(grad, x, table, off_d, res_d, ge, N, D, Cc, L)
    assert _tail_kept(ge, rows * Cc)
    return ge[:rows * Cc].view(rows, Cc)


def test_one_chunk_pipeline_trips_and_order_independence():
    """(e) deterministic mode: one chunk of all N points per (level, slice), N around one, two and several trips of the two-point
    pipeline (1024 threads x 2 points).  Two launches give the same bits; so does a launch on a permutation of the points (gradient
    rows permuted with them): the 64-bit fixed-point sums are exact, the one float add per word is the only rounding.  The rule
    against the statement at every N."""
    lb, Lh, st = _lib()
    D, Cc, res = 3, 8, (18, 40)
    off = _levels(D, res, 13)
    L, rows = 2, off[-1]
    off_d, res_d = _i32dev(off), _i32dev(res)
    Lh.gsvc_set_deterministic(1)
    try:
        for N in (1023, 1024, 1025, 2047, 2048, 2049, 4096, 5000):
            x, table, grad = (_dev(a) for a in grid_case(D, Cc, off, res, N, N))
            a = _table_grad(grad, x, off_d, res_d, rows, N, D, Cc, L, table)
            b = _table_grad(grad, x, off_d, res_d, rows, N, D, Cc, L, table)
            perm = torch.randperm(N, generator=torch.Generator().manual_seed(N)).cuda()
            c = _table_grad(grad[:, perm].contiguous(), x[perm].contiguous(), off_d, res_d, rows, N, D, Cc, L, table)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            assert torch.equal(a.view(torch.int32), c.view(torch.int32))
            Refs(x, table, off, res, grad).check_table_grad(f"e one chunk N={N}", a)
    finally:
        Lh.gsvc_set_deterministic(0)


def test_four_chunks_in_default_mode():
    """(e) N = 6200, L = 2, D = 3: min(256 / (2 * 4), ceil(6200 / 2048)) = 4 chunks of 1550 points, four float adds per word."""
    D, Cc, res, N = 3, 8, (18, 40), 6200
    off = _levels(D, res, 13)
    x, table, grad = (_dev(a) for a in grid_case(D, Cc, off, res, N, 5))
    got = _table_grad(grad, x, _i32dev(off), _i32dev(res), off[-1], N, D, Cc, 2, table)
    Refs(x, table, off, res, grad).check_table_grad("e four chunks", got)


# ---------------------------------------------------------------------------------------------------------------- (f) scales
MAGS = (1e3, 1.0, 1e-12, 1e-25)          # 1e-25 < 2^-60: that level takes the float path


def test_scales_per_level_and_a_small_channel():
    """(f) the four levels of one grid carry gradients of magnitude 1e3, 1, 1e-12 and 1e-25, and channel 1 lies six orders of
    magnitude below its level's largest: every (level, channel) block holds the rule on its own scale."""
    D, Cc, res, N = 3, 8, (18, 24, 33, 44), 4000
    off = _levels(D, res, 13)
    x, table, grad = grid_case(D, Cc, off, res, N, 17)
    for l, m in enumerate(MAGS):
        grad[l] *= np.float32(m)
    grad[..., 1] *= np.float32(1e-6)
    x, table, grad = _dev(x), _dev(table), _dev(grad)
    got = _table_grad(grad, x, _i32dev(off), _i32dev(res), off[-1], N, D, Cc, 4, table)
    r = Refs(x, table, off, res, grad)
    r.check_table_grad("f scales", got)
    for l in range(4):                    # and block by block, so that a small block cannot hide behind a large one
        for ch in range(Cc):
            blk = (slice(off[l], off[l + 1]), slice(ch, ch + 1))
            sc = float(r.s_gt[off[l], ch])
            assert sc > 0
            _rule(f"f level {l} channel {ch}", err(got[blk], r.gt64[blk], sc), err(r.gt32[blk], r.gt64[blk], sc))


def test_ring_of_level_maxima_is_reused_after_32_calls():
    """(f) 33 backward calls in a row on one stream, magnitudes alternating between 1e6 and 1e-6: call 33 takes the ring slot of
    call 1 with the other magnitude.  A stale maximum would cost 2^40 in resolution or overflow the fixed-point words."""
    D, Cc, res, N = 3, 8, (18, 24), 64
    off = _levels(D, res, 13)
    x, table, grad = grid_case(D, Cc, off, res, N, 3)
    x, table = _dev(x), _dev(table)
    off_d, res_d = _i32dev(off), _i32dev(res)
    grads = [_dev(grad * np.float32(m)) for m in (1e6, 1e-6)]
    refs = [Refs(x, table, off, res, g) for g in grads]
    bufs = []
    for k in range(33):
        ge = _zeros_guarded(off[-1] * Cc)
        _backward(grads[k % 2], x, table, off_d, res_d, ge, N, D, Cc, 2)
        bufs.append(ge)
    for k, ge in enumerate(bufs):
        assert _tail_kept(ge, off[-1] * Cc)
        refs[k % 2].check_table_grad(f"f ring call {k + 1}", ge[:off[-1] * Cc].view(off[-1], Cc))


# ---------------------------------------------------------------------------------------------------------------- (g) _ex
def _points5(N, seed):
    """[N, 5] uniform points; rows 0-4 as in grid_case (all 0, all 1, one coordinate outside in rows 2 and 3, all 0.5)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (N, 5)).astype(np.float32)
    x[0], x[1], x[4] = 0.0, 1.0, 0.5
    x[2, 3] = -0.1             # first coordinate of the 3-D grid below
    x[3, 1] = 1.0001           # last coordinate of the 2-D grid
    x[7] = x[8]
    return _dev(x)


def _forward_ex(xmat, table, off_d, res_d, feat, base, N, D, Cc, L, io):
    lb, Lh, st = _lib()
    lb.check(Lh.gsvc_grid_forward_ex(_p(xmat), _p(table), _p(off_d), _p(res_d), _p(feat[base:]), N, D, Cc, L, C.byref(_ioc(io)), st),
             "gsvc_grid_forward_ex")


def _backward_ex(gmat, base, xmat, off_d, res_d, ge, N, D, Cc, L, io):
    lb, Lh, st = _lib()
    lb.check(Lh.gsvc_grid_backward_ex(_p(gmat[base:]), _p(xmat), _p(off_d), _p(res_d), _p(ge), N, D, Cc, L, C.byref(_ioc(io)), st),
             "gsvc_grid_backward_ex")


def test_ex_layouts_write_and_read_only_their_block():
    """(g) one [N, 40] feature matrix holds a 3-D grid's block at columns 8..23 and a 2-D grid's at 24..39 (C = 8, two levels each);
    the points are columns (3, 0, 2) and (4, 1) of an [N, 5] matrix.  After each forward call everything outside the block written
    still holds the NaN pattern or the other grid's bits; the blocks hold the statement's features.  The gradient matrix carries
    the NaN pattern in columns 0..7: the table gradients read from the strided blocks are the statement's."""
    N, Cc, L, W = 3000, 8, 2, 40
    xmat = _points5(N, 21)
    grids = [dict(D=3, res=(18, 40), log2=13, base=8, io=GridIO(Cc, W, 5, (3, 0, 2))), dict(D=2, res=(130, 258), log2=15, base=24, io=GridIO(Cc, W, 5, (4, 1)))]
    feat = _sentinel(N * W)
    rng = np.random.default_rng(22)
    gmat = _sentinel(N * W)
    for g in grids:
        g["off"] = _levels(g["D"], g["res"], g["log2"])
        g["table"] = _dev(rng.standard_normal((g["off"][-1], Cc)).astype(np.float32))
        g["x"] = io_points(xmat, g["io"], g["D"])
        g["grad"] = _dev(rng.standard_normal((L, N, Cc)).astype(np.float32))
        io_place(gmat, g["base"], g["io"], g["grad"])
        g["ref"] = Refs(g["x"], g["table"], g["off"], g["res"], g["grad"])
        assert int(g["ref"].outside.sum()) == 1
    expect = feat.clone()
    for g in grids:
        _forward_ex(xmat, g["table"], _i32dev(g["off"]), _i32dev(g["res"]), feat, g["base"], N, g["D"], Cc, L, g["io"])
        got = io_extract(feat, g["base"], g["io"], L, N, Cc)
        g["ref"].check_forward(f"g ex D={g['D']}", got)
        io_place(expect, g["base"], g["io"], got)
        assert torch.equal(feat.view(torch.int32), expect.view(torch.int32))          # nothing else moved
    m = feat[:N * W].view(N, W).view(torch.int32)
    assert bool((m[:, :8] == SENTINEL).all()) and bool((m[:, 8:] != SENTINEL).all())
    gm = gmat[:N * W].view(N, W).view(torch.int32)
    assert bool((gm[:, :8] == SENTINEL).all()) and bool((gm[:, 8:] != SENTINEL).all())
    for g in grids:
        rows = g["off"][-1]
        ge = _zeros_guarded(rows * Cc)
        _backward_ex(gmat, g["base"], xmat, _i32dev(g["off"]), _i32dev(g["res"]), ge, N, g["D"], Cc, L, g["io"])
        assert _tail_kept(ge, rows * Cc)
        g["ref"].check_table_grad(f"g ex D={g['D']}", ge[:rows * Cc].view(rows, Cc))


# ---------------------------------------------------------------------------------------------------------------- (h) _many
def _many_setup(n_jobs, Cc, N, seed):
    """A 3-D grid of 3 levels, then 2-D grids of 4 levels on the column pairs (0, 1), (0, 2), (1, 2) of x [N, 3]; the blocks lie
    in one [N, W] matrix, 4 or more sentinel columns before, between and after them, every block starting on a 16-byte boundary."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    x[0], x[1], x[4] = 0.0, 1.0, 0.5
    x[2, 0], x[3, 2] = -0.1, 1.0001
    x[7] = x[8]
    xmat = _dev(x)
    specs = [(3, (18, 24, 33), 13, (0, 1, 2)), (2, (130, 258, 514, 1026), 15, (0, 1)), (2, (130, 258, 514, 1026), 15, (0, 2)),
             (2, (130, 258, 514, 1026), 15, (1, 2))][:n_jobs]
    col, grids = 4, []
    for D, res, log2, cols in specs:
        grids.append(dict(D=D, res=res, L=len(res), off=_levels(D, res, log2), base=col, cols=cols))
        col += len(res) * Cc
        col += 4 + (-col) % 4
    W = col
    first = 0
    for g in grids:
        g["io"] = GridIO(Cc, W, 3, g["cols"])
        g["table"] = _dev(rng.standard_normal((g["off"][-1], Cc)).astype(np.float32))
        g["x"] = io_points(xmat, g["io"], g["D"])
        grad = rng.standard_normal((g["L"], N, Cc)).astype(np.float32)
        for l in range(g["L"]):
            grad[l] *= np.float32(MAGS[(first + l + len(grids)) % 4])          # every (grid, level) its own magnitude
        first += g["L"]
        g["grad"] = _dev(grad)
        g["off_d"], g["res_d"] = _i32dev(g["off"]), _i32dev(g["res"])
    return xmat, grids, W


def _many_jobs(grids, feat, backward):
    from gsvc_amd import _lib
    jobs = (_lib.GridManyJobC * len(grids))()
    for j, g in zip(jobs, grids):
        j.embeddings = None if backward else _p(g["table"])
        j.features = _p(feat[g["base"]:])
        j.grad_embeddings = _p(g["ge"]) if backward else None
        j.offsets, j.resolutions = _p(g["off_d"]), _p(g["res_d"])
        j.D, j.L, j.layout = g["D"], g["L"], _ioc(g["io"])
    return jobs


@pytest.mark.parametrize("n_jobs", [1, 2, 4])
@pytest.mark.parametrize("Cc", [2, 4, 8])
def test_many_grids_in_one_launch(n_jobs, Cc):
    """(h) N = 10300: the 3-D grid gets min(256 / (3 * 4), ceil(N / 2048)) = 6 chunks, a 2-D grid min(256 / (4 * 16), 6) = 4, so the
    2-D grids' workgroups with blockIdx.x >= 4 return early.  The forward matrix is gsvc_grid_forward_ex's per grid bit for bit,
    sentinel columns included; the features and the table gradients hold the rule, every (grid, level) with its own gradient
    magnitude (a level maximum read from another level's row of the slot loses the small levels or overflows the large ones)."""
    lb, Lh, st = _lib()
    N = 10300
    xmat, grids, W = _many_setup(n_jobs, Cc, N, 100 * n_jobs + Cc)
    feat, feat_ex = _sentinel(N * W), _sentinel(N * W)
    lb.check(Lh.gsvc_grid_forward_many(_p(xmat), _many_jobs(grids, feat, False), n_jobs, N, Cc, st), "gsvc_grid_forward_many")
    for g in grids:
        _forward_ex(xmat, g["table"], g["off_d"], g["res_d"], feat_ex, g["base"], N, g["D"], Cc, g["L"], g["io"])
    assert torch.equal(feat.view(torch.int32), feat_ex.view(torch.int32))
    written = torch.zeros(W, dtype=torch.bool, device="cuda")
    for g in grids:
        written[g["base"]:g["base"] + g["L"] * Cc] = True
    m = feat[:N * W].view(N, W).view(torch.int32)
    assert bool((m[:, ~written] == SENTINEL).all()) and bool((m[:, written] != SENTINEL).all()) and _tail_kept(feat, N * W)
    assert int((~written).sum()) >= 4 * (n_jobs + 1)
    gmat = _sentinel(N * W)
    for g in grids:
        g["ref"] = Refs(g["x"], g["table"], g["off"], g["res"], g["grad"])
        g["ref"].check_forward(f"h many jobs={n_jobs} C={Cc} D={g['D']} cols={g['cols']}", io_extract(feat, g["base"], g["io"], g["L"], N, Cc))
        io_place(gmat, g["base"], g["io"], g["grad"])
        g["ge"] = _zeros_guarded(g["off"][-1] * Cc)
    lb.check(Lh.gsvc_grid_backward_many(_p(xmat), _many_jobs(grids, gmat, True), n_jobs, N, Cc, st), "gsvc_grid_backward_many")
    for g in grids:
        rows = g["off"][-1]
        assert _tail_kept(g["ge"], rows * Cc)
        g["ref"].check_table_grad(f"h many jobs={n_jobs} C={Cc} D={g['D']} cols={g['cols']}", g["ge"][:rows * Cc].view(rows, Cc))


# ---------------------------------------------------------------------------------------------------------------- (i) packed
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_pack_sign_bits(rows):
    """bits[row] bit f = (x[row, f] >= 0) with 0.0, -0.0 (both >= 0), the smallest negative normal and a negative subnormal in the
    data; nothing past the last row is written."""
    lb, Lh, st = _lib()
    rng = np.random.default_rng(rows)
    x = rng.standard_normal((rows, 8)).astype(np.float32)
    edge = np.array([0.0, -0.0, -1.1754944e-38, -1e-40, 1e-40, -1e-30, 1e-30, -1.0], dtype=np.float32)
    x[0] = edge
    x[rows - 1] = edge[::-1] if rows > 1 else edge
    x.reshape(-1)[::13] = -0.0
    want = np.packbits(x >= 0, axis=1, bitorder="little").reshape(-1)
    buf = torch.full((rows + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    xd = _dev(x)
    lb.check(Lh.gsvc_pack_sign_bits(_p(xd), rows, _p(buf), st), "gsvc_pack_sign_bits")
    assert np.array_equal(buf[:rows].cpu().numpy(), want) and bool((buf[rows:] == 0xA5).all())
    assert want[0] == 0b01010011


@pytest.mark.parametrize("D,res,log2,cols", [(3, (18, 24, 33), 13, (3, 0, 2)), (2, (130, 258), 15, (4, 1))])
def test_packed_forward_is_the_float_lookup(D, res, log2, cols):
    """gsvc_grid_forward_packed on the bytes gsvc_pack_sign_bits makes of a float table equals gsvc_grid_forward_ex on the +-1 float
    table bit for bit: with the default layout (NULL) and in a column block of an [N, 40] matrix with permuted input columns."""
    lb, Lh, st = _lib()
    N, Cc, L, W = 3000, 8, len(res), 40
    off = _levels(D, res, log2)
    off_d, res_d = _i32dev(off), _i32dev(res)
    rng = np.random.default_rng(D)
    raw = rng.standard_normal((off[-1], Cc)).astype(np.float32)
    raw[::7] = 0.0
    raw[::11] = -0.0
    raw = _dev(raw)
    table = torch.where(raw >= 0, 1.0, -1.0).contiguous()
    bits = torch.zeros(off[-1] + 16, dtype=torch.uint8, device="cuda")
    lb.check(Lh.gsvc_pack_sign_bits(_p(raw), off[-1], _p(bits), st), "gsvc_pack_sign_bits")
    xmat = _points5(N, 40 + D)
    # default layout: points [N, D] dense
    x = io_points(xmat, GridIO(Cc, W, 5, cols), D)
    io = io_default(N, D, Cc)
    a, b = _sentinel(L * N * Cc), _sentinel(L * N * Cc)
    lb.check(Lh.gsvc_grid_forward_packed(_p(x), _p(bits), _p(off_d), _p(res_d), _p(a), N, D, L, None, st), "gsvc_grid_forward_packed")
    _forward_ex(x, table, off_d, res_d, b, 0, N, D, Cc, L, io)
    assert _written(a, L * N * Cc) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    Refs(x, table, off, res).check_forward(f"i packed D={D}", a[:L * N * Cc].view(L, N, Cc))
    # strided: the block at column 16 of [N, 40]
    io = GridIO(Cc, W, 5, cols)
    a, b = _sentinel(N * W), _sentinel(N * W)
    lb.check(Lh.gsvc_grid_forward_packed(_p(xmat), _p(bits), _p(off_d), _p(res_d), _p(a[16:]), N, D, L, C.byref(_ioc(io)), st), "gsvc_grid_forward_packed")
    _forward_ex(xmat, table, off_d, res_d, b, 16, N, D, Cc, L, io)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    m = a[:N * W].view(N, W).view(torch.int32)
    assert bool((m[:, :16] == SENTINEL).all()) and bool((m[:, 16:16 + L * Cc] != SENTINEL).all()) and bool((m[:, 16 + L * Cc:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- (j) refusals
def test_refusals_and_empty_calls_launch_nothing():
    """Every refusal below returns from the entry point before its launch (grid_io_from / grid_many_fill / the C switch of the
    _many entries / the argument checks of the packed entries): the error is raised and every buffer still holds the NaN pattern.
    N = 0 and L = 0 return OK without a launch on the single-grid entries; a _many job needs at least one level (its contract in
    include/gsvc_hip.h), so there L = 0 is a refusal and N = 0 the empty call."""
    lb, Lh, st = _lib()
    N, Cc, L, W = 64, 8, 2, 40
    off3, off2 = _levels(3, (18, 24), 13), _levels(2, (18, 34), 12)
    res3, res2 = _i32dev((18, 24)), _i32dev((18, 34))
    o3, o2 = _i32dev(off3), _i32dev(off2)
    xmat = _points5(N, 1)
    t3 = torch.ones(off3[-1], Cc, device="cuda")
    bits = torch.zeros(off3[-1] + 16, dtype=torch.uint8, device="cuda")
    feat, ge, out1 = _sentinel(N * W), _sentinel(off3[-1] * Cc), _sentinel(4 * N * 16)
    gsrc = torch.ones(N * W + PAD, device="cuda")
    good = GridIO(Cc, W, 5, (3, 0, 2))

    def many(io=good, D=3, Ljob=L, backward=False, n=1, Cm=Cc, Nn=N):
        from gsvc_amd import _lib
        jobs = (_lib.GridManyJobC * 5)()
        for j in jobs:
            j.embeddings, j.features, j.grad_embeddings = _p(t3), _p((gsrc if backward else feat)[8:]), _p(ge)
            j.offsets, j.resolutions, j.D, j.L, j.layout = _p(o3), _p(res3), D, Ljob, _ioc(io)
        fn = Lh.gsvc_grid_backward_many if backward else Lh.gsvc_grid_forward_many
        return fn(_p(xmat), jobs, n, Nn, Cm, st)

    bad_layouts = [(GridIO(Cc, Cc - 1, 5, (3, 0, 2)), "bad layout"), (GridIO(Cc, W + 2, 5, (3, 0, 2)), "feature strides must be multiples of 4 floats"),
                   (GridIO(Cc + 2, W, 5, (3, 0, 2)), "feature strides must be multiples of 4 floats"),
                   (GridIO(Cc, W, 5, (3, 5, 2)), "input column outside the row"), (GridIO(Cc, W, 5, (-1, 0, 2)), "input column outside the row"),
                   (GridIO(Cc, W, 0, (0, 0, 0)), "bad layout")]
    for io, msg in bad_layouts:
        ioc = _ioc(io)
        with pytest.raises(lb.GsvcError, match=msg):
            lb.check(Lh.gsvc_grid_forward_ex(_p(xmat), _p(t3), _p(o3), _p(res3), _p(feat[8:]), N, 3, Cc, L, C.byref(ioc), st), "forward_ex")
        with pytest.raises(lb.GsvcError, match=msg):
            lb.check(Lh.gsvc_grid_backward_ex(_p(gsrc[8:]), _p(xmat), _p(o3), _p(res3), _p(ge), N, 3, Cc, L, C.byref(ioc), st), "backward_ex")
        with pytest.raises(lb.GsvcError, match=msg):
            lb.check(Lh.gsvc_grid_forward_packed(_p(xmat), _p(bits), _p(o3), _p(res3), _p(feat[8:]), N, 3, L, C.byref(ioc), st), "forward_packed")
        for backward in (False, True):
            with pytest.raises(lb.GsvcError, match=msg):
                lb.check(many(io=io, backward=backward), "many")
    # C = 2: strides must be multiples of 2
    with pytest.raises(lb.GsvcError, match="feature strides must be multiples of 2 floats"):
        lb.check(Lh.gsvc_grid_forward_ex(_p(xmat), _p(t3), _p(o3), _p(res3), _p(feat[8:]), N, 3, 2, L, C.byref(_ioc(GridIO(2, 41, 5, (3, 0, 2)))), st), "forward_ex")
    for backward in (False, True):
        for kw, msg in ((dict(n=0), "1..4 grids"), (dict(n=5), "1..4 grids"), (dict(D=1), "grids of 2 or 3 dimensions"),
                        (dict(Ljob=0), "at least one level"), (dict(Cm=1), "2, 4 or 8 features per level"), (dict(Cm=16), "2, 4 or 8 features per level")):
            with pytest.raises(lb.GsvcError, match=msg):
                lb.check(many(backward=backward, **kw), "many")
        lb.check(many(backward=backward, Nn=0), "many N=0")
    with pytest.raises(lb.GsvcError, match="num_dim must be 2 or 3"):
        lb.check(Lh.gsvc_grid_forward_packed(_p(xmat), _p(bits), _p(o3), _p(res3), _p(out1), N, 1, L, None, st), "forward_packed")
    with pytest.raises(lb.GsvcError, match="pack_sign_bits: bad size"):
        lb.check(Lh.gsvc_pack_sign_bits(_p(t3), -1, _p(out1.view(torch.uint8)), st), "pack_sign_bits")
    # unsupported sizes of the single-grid entries
    with pytest.raises(lb.GsvcError, match="num_dim must be 1, 2, 3"):
        lb.check(Lh.gsvc_grid_forward(_p(xmat), _p(t3), _p(o3), _p(res3), _p(out1), N, 4, Cc, L, None, st), "forward")
    with pytest.raises(lb.GsvcError, match="n_fearures must be 1, 2, 4, 8, 16 or 32"):
        lb.check(Lh.gsvc_grid_backward(_p(gsrc), _p(xmat), _p(t3), _p(o3), _p(res3), _p(ge), N, 3, 3, L, None, None, st), "backward")
    # empty calls
    for Nn, Ln in ((0, L), (N, 0), (0, 0)):
        ioc = _ioc(good)
        lb.check(Lh.gsvc_grid_forward(_p(xmat), _p(t3), _p(o3), _p(res3), _p(out1), Nn, 3, Cc, Ln, _p(feat), st), "forward")
        lb.check(Lh.gsvc_grid_backward(_p(gsrc), _p(xmat), _p(t3), _p(o3), _p(res3), _p(ge), Nn, 3, Cc, Ln, _p(gsrc), _p(out1), st), "backward")
        lb.check(Lh.gsvc_grid_forward_ex(_p(xmat), _p(t3), _p(o3), _p(res3), _p(feat[8:]), Nn, 3, Cc, Ln, C.byref(ioc), st), "forward_ex")
        lb.check(Lh.gsvc_grid_backward_ex(_p(gsrc[8:]), _p(xmat), _p(o3), _p(res3), _p(ge), Nn, 3, Cc, Ln, C.byref(ioc), st), "backward_ex")
        lb.check(Lh.gsvc_grid_forward_packed(_p(xmat), _p(bits), _p(o3), _p(res3), _p(feat[8:]), Nn, 3, Ln, C.byref(ioc), st), "forward_packed")
        lb.check(Lh.gsvc_grid_forward_packed(_p(xmat), _p(bits), _p(o2), _p(res2), _p(out1), Nn, 2, Ln, None, st), "forward_packed")
    lb.check(Lh.gsvc_pack_sign_bits(_p(t3), 0, _p(out1.view(torch.uint8)), st), "pack_sign_bits")
    torch.cuda.synchronize()
    assert _untouched(feat) and _untouched(ge) and _untouched(out1) and not bits.any() and bool((gsrc == 1).all())
