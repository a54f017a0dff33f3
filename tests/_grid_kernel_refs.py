"""Plain tensor statement of the multi-resolution hash-grid encoder, written from the header comment of csrc/grid.hip and the
contract of include/gsvc_hip.h.  Called with dtype = float64 it is the reference of tests/test_grid_kernels_gpu.py; called with
float32 it is "the fp32 tensor statement" those tests calibrate against.  tests/test_grid_kernel_refs_cpu.py pins it without a
GPU.  Nothing here imports the package under test or the oracle.

The discrete decisions are inputs of the operation: which cell a point falls into and its fractional position inside it are formed
in float32 exactly as the contract states them (one rounded product, one rounded sum, floor; the difference is exact in fp32), and
only then cast up.  Everything that follows (corner weights, renormalisation, interpolation, finite differences, scatter-add) runs
in ``dtype``.
"""
from collections import namedtuple

import numpy as np
import torch

from tests._step_kernel_refs import EPS32, PRINT, err, err_each  # noqa: F401  (re-exported for the tests)

HASH_PRIMES = (1, 2654435761, 805459861)
_M32 = 0xFFFFFFFF

# gsvc_grid_io: feature (level l, point b, channel c) at l * feat_level_stride + b * feat_point_stride + c floats past the block's
# base; coordinate d of point b at column in_col[d] of a row-major [N, in_stride] matrix
GridIO = namedtuple("GridIO", "feat_level_stride feat_point_stride in_stride in_col")


def grid_rows(p, res, rows):
    """Table row of the integer grid positions ``p`` [..., D] (int64) on a level of resolution ``res`` with ``rows`` table rows:
    the dense index sum_d p[d] res^d while the running stride (1, res, res^2, ...) stays <= rows in every dimension, else the XOR of
    p[d] * {1, 2654435761, 805459861} in 32-bit unsigned arithmetic; then modulo ``rows``."""
    D = p.shape[-1]
    stride, index = 1, torch.zeros_like(p[..., 0])
    for d in range(D):
        if stride <= rows:
            index = (index + p[..., d] * stride) & _M32
            stride = (stride * res) & _M32
    if stride > rows:
        index = torch.zeros_like(index)
        for d in range(D):
            index = index ^ ((p[..., d] * HASH_PRIMES[d]) & _M32)
    return index % rows


def grid_cells(x, res):
    """(cell [N, D] int64, frac [N, D] float32) of float32 points on a level: pos = fl32(fl32(x * (res - 2)) + 0.5), cell = floor(pos),
    frac = pos - cell (exact in float32).  Two tensor operations, so nothing is contracted into a fused multiply-add."""
    x = x.to(torch.float32)
    pos = x * torch.tensor(float(res - 2), dtype=torch.float32, device=x.device)
    pos = pos + torch.tensor(0.5, dtype=torch.float32, device=x.device)
    cell = torch.floor(pos)
    return cell.to(torch.int64), pos - cell


def grid_forward_ref(x, table, offsets, resolutions, dtype):
    """x [N, D] float32, table [rows, C], offsets [L + 1] and resolutions [L] (host integers).
    Returns out [L, N, C], dy_dx [N, L, D, C] and, per level, ``dict(rows, w, valid)`` of [N, 2^D] tensors: the level-local table
    row of every corner (0 where dropped), its renormalised weight (0 where dropped) and whether it takes part.  Corner ``idx`` takes
    the upper neighbour in dimension d when bit d of idx is set."""
    offsets, resolutions = [int(o) for o in offsets], [int(r) for r in resolutions]
    N, D = x.shape
    C, L, dev = table.shape[1], len(resolutions), x.device
    tab = table.to(dtype)
    oob = ((x < 0) | (x > 1)).any(dim=1)
    out = torch.zeros(L, N, C, dtype=dtype, device=dev)
    dy_dx = torch.zeros(N, L, D, C, dtype=dtype, device=dev)
    located = []
    for l, res in enumerate(resolutions):
        rows = offsets[l + 1] - offsets[l]
        cell, frac = grid_cells(x, res)
        cell = torch.where(oob[:, None], torch.zeros_like(cell), cell)       # (an outside point takes no part; keep its indices tame)
        frac = frac.to(dtype)
        raw_w, valid, row, g = [], [], [], []
        for idx in range(1 << D):
            w = torch.ones(N, dtype=dtype, device=dev)
            pl = []
            for d in range(D):
                if (idx >> d) & 1:
                    w = w * frac[:, d]
                    pl.append(torch.clamp(cell[:, d] + 1, max=res - 1))
                else:
                    w = w * (1 - frac[:, d])
                    pl.append(cell[:, d])
            p = torch.stack(pl, dim=1)
            ok = ~((p == 0) | (p == res - 1)).any(dim=1) & ~oob
            r = torch.where(ok, grid_rows(p, res, rows), torch.zeros_like(p[:, 0]))
            raw_w.append(w)
            valid.append(ok)
            row.append(r)
            g.append(tab[offsets[l] + r] * ok[:, None].to(dtype))            # a dropped corner reads as 0
        wn = torch.zeros(N, dtype=dtype, device=dev)
        for w, ok in zip(raw_w, valid):
            wn = wn + torch.where(ok, w, torch.zeros_like(w))
        wn = torch.where(wn == 0, torch.full_like(wn, 1e-9), wn)
        wnorm = [torch.where(ok, w / wn, torch.zeros_like(w)) for w, ok in zip(raw_w, valid)]
        for w, gi in zip(wnorm, g):
            out[l] += w[:, None] * gi
        for gd in range(D):
            acc = torch.zeros(N, C, dtype=dtype, device=dev)
            for lo in range(1 << D):
                if (lo >> gd) & 1:
                    continue
                w = torch.full((N,), float(res - 2), dtype=dtype, device=dev)
                for d in range(D):
                    if d != gd:
                        w = w * (frac[:, d] if (lo >> d) & 1 else 1 - frac[:, d])
                acc = acc + w[:, None] * (g[lo | (1 << gd)] - g[lo])
            dy_dx[:, l, gd] = acc
        located.append(dict(rows=torch.stack(row, 1), w=torch.stack(wnorm, 1), valid=torch.stack(valid, 1)))
    return out, dy_dx, located


def grid_backward_ref(grad, located, offsets, C, dy_dx, dtype, prior=None):
    """grad [L, N, C]; ``located`` from grid_forward_ref run in the same dtype.  Returns (table gradient [offsets[-1], C]: the
    scatter-add of weight * grad over the valid corners; counts [offsets[-1]] int64: how many contributions each row's C words
    received; grad_inputs [N, D] = sum_l sum_c grad[l, b, c] dy_dx[b, l, d, c], None without dy_dx).  With ``prior`` [offsets[-1], C]
    the contributions are added onto a copy of it (the entry points accumulate into the caller's table gradient)."""
    offsets = [int(o) for o in offsets]
    dev = grad.device
    gt = torch.zeros(offsets[-1], C, dtype=dtype, device=dev) if prior is None else prior.to(dtype).clone()
    counts = torch.zeros(offsets[-1], dtype=torch.int64, device=dev)
    for l, loc in enumerate(located):
        b, k = loc["valid"].nonzero(as_tuple=True)
        target = offsets[l] + loc["rows"][b, k]
        gt.index_add_(0, target, loc["w"].to(dtype)[b, k][:, None] * grad[l].to(dtype)[b])
        counts.index_add_(0, target, torch.ones_like(target))
    gi = None if dy_dx is None else torch.einsum("lbc,bldc->bd", grad.to(dtype), dy_dx.to(dtype))
    return gt, counts, gi


# ------------------------------------------------------------------------------------------------------------ strided layouts
def io_default(N, D, C):
    """The layout of gsvc_grid_forward / gsvc_grid_backward: points [N, D] dense, features [L, N, C]."""
    return GridIO(N * C, C, D, tuple(range(D)))


def io_view(buf, base, io, L, N, C):
    """The [L, N, C] view of a grid's feature block inside the flat float buffer ``buf``, the block starting ``base`` floats in."""
    return buf.view(-1).as_strided((L, N, C), (io.feat_level_stride, io.feat_point_stride, 1), base)


def io_place(buf, base, io, block):
    """Writes block [L, N, C] into its place; every other element of ``buf`` keeps its value."""
    L, N, C = block.shape
    io_view(buf, base, io, L, N, C).copy_(block)


def io_extract(buf, base, io, L, N, C):
    return io_view(buf, base, io, L, N, C).clone()


def io_points(xmat, io, D):
    """The [N, D] points a grid reads from the row-major matrix ``xmat`` of ``io.in_stride`` columns."""
    return xmat.view(-1, io.in_stride)[:, list(io.in_col[:D])].contiguous()


# ------------------------------------------------------------------------------------------------------------ test inputs
def grid_case(D, C, offsets, resolutions, N, seed):
    """(x [N, D], table [offsets[-1], C], grad [L, N, C]) as float32 numpy arrays from numpy.default_rng(seed): a standard-normal
    table and gradient, points uniform in [0, 1]^D and, as far as N allows, row 0 all 0, row 1 all 1, row 2 with its first
    coordinate -0.1, row 3 with its last coordinate 1.0001, row 4 all 0.5, rows 5 and 6 inside the first and the last interior cell
    of the coarsest level (above resolution 2), row 7 a copy of row 8."""
    rng = np.random.default_rng(seed)
    table = rng.standard_normal((int(offsets[-1]), C)).astype(np.float32)
    x = rng.uniform(0, 1, (N, D)).astype(np.float32)
    grad = rng.standard_normal((len(resolutions), N, C)).astype(np.float32)
    s = float(min(int(r) for r in resolutions if int(r) > 2) - 2)
    special = [np.zeros(D), np.ones(D), None, None, np.full(D, 0.5), np.full(D, 0.8 / s), np.full(D, (s - 0.2) / s)]
    for i, row in enumerate(special):
        if i < N and row is not None:
            x[i] = row
    if N > 2:
        x[2, 0] = -0.1
    if N > 3:
        x[3, -1] = 1.0001
    if N > 8:
        x[7] = x[8]
    return x, table, grad
