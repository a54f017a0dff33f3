"""The hash-grid statement of tests/_grid_kernel_refs.py pinned on its own, without a GPU: a wrong reference must not be able to
bless a wrong kernel.  In float64 against the reference implementation's own numbers (tests/golden/grid_encoder_{3d,2d}.npz) and
against the fp32 CPU oracle at the small shapes of tests/test_grid_kernels_gpu.py, the row indices against values worked out by
hand, the scatter-add against float64 autograd of an independent gather, dy_dx against the derivative of the interpolation.

Bounds: 4 eps32 of the scale for features, dy_dx and input gradients, 8 eps32 of the largest entry for table gradients.  Both
comparands other than the statement are fp32 evaluations stored in fp32: a feature is a sum of at most 8 products of a weight
(3 roundings) with a table entry, a table-gradient entry a longer fp32 sum.
"""
import os

import numpy as np
import pytest
import torch

from tests._grid_kernel_refs import EPS32, PRINT, err, grid_backward_ref, grid_case, grid_cells, grid_forward_ref, grid_rows

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def T(a):
    return torch.from_numpy(np.asarray(a))


def _levels(D, res, log2):
    from gsvc_amd.encodings import level_offsets
    return level_offsets(res, D, log2)


@pytest.mark.parametrize("tag", ["3d", "2d"])
def test_statement_reproduces_the_reference_fixture(tag):
    """float64 statement on the fixture's points and binarised tables against the reference GridEncoder's fp32 out, dx and dparams
    (the straight-through mask |params| <= 1 is applied here, it is no part of the statement).
    measured: out 2.1e-7 (3-D) / 1.2e-7 (2-D) absolute, dx 8.9e-8 / 1.1e-7, dparams 1.2e-7 / 6.7e-8 of the largest entry."""
    g = np.load(os.path.join(GOLD, f"grid_encoder_{tag}.npz"), allow_pickle=False)
    params, x = T(g["params"]), T(g["x"])
    table = torch.where(params >= 0, 1.0, -1.0)
    (N, D), C, L = x.shape, params.shape[1], len(g["resolutions"])
    out, dy_dx, located = grid_forward_ref(x, table, g["offsets"], g["resolutions"], torch.float64)
    grad = T(g["gout"]).view(N, L, C).permute(1, 0, 2).contiguous()
    gt, _, gi = grid_backward_ref(grad, located, g["offsets"], C, dy_dx, torch.float64)
    e_out = err(out.permute(1, 0, 2).reshape(N, L * C), T(g["out"]), 1.0)
    e_dx = err(gi, T(g["dx"]), float(np.abs(g["dx"]).max()))
    e_dp = err(gt * (params.abs() <= 1), T(g["dparams"]), float(np.abs(g["dparams"]).max()))
    if PRINT:
        print(f"GRID_REF fixture {tag}: out {e_out:.3e} dx {e_dx:.3e} dparams {e_dp:.3e}")
    assert e_out <= 4 * EPS32 and e_dx <= 4 * EPS32 and e_dp <= 8 * EPS32


# (D, C, resolutions, offsets): the forward shapes of the GPU test, a hashed table that is no power of two, and a level of
# resolution 2 (every corner of every point lies on the border: the level's features are zero)
def _oracle_cases():
    shapes = [(1, 1, (16, 64), 5), (2, 2, (10, 18), 8), (3, 4, (6, 9, 14), 9), (3, 8, (18, 24, 33, 44), 13), (2, 8, (130, 258), 15),
              (3, 16, (18, 40), 11), (2, 32, (20,), 7)]
    cases = [(D, C, res, _levels(D, res, log2)) for D, C, res, log2 in shapes]
    cases.append((3, 2, (40, 57), [0, 1000, 2000]))
    cases.append((2, 2, (2, 10), [0, 8, 112]))
    return cases


@pytest.mark.parametrize("N", [1, 257, 3000])
def test_statement_against_the_cpu_oracle(oracle_lib, N):
    """Features, dy_dx, table gradient and input gradient of the float64 statement against oracle/grid_oracle.c (fp32, the kernel's
    operation order) per level on the scales of the GPU test; rows of points outside [0, 1]^D, and the level whose corners all lie
    on the border, are exactly zero in both.
    measured, largest over the cases: out 2.0e-7, dy_dx 2.1e-7, table gradient 5.1e-7, input gradient 2.3e-7."""
    worst = dict(out=0.0, dy_dx=0.0, table=0.0, inputs=0.0)
    for k, (D, C, res, off) in enumerate(_oracle_cases()):
        x, table, grad = grid_case(D, C, off, res, N, 100 * k + D)
        L = len(res)
        out, dy_dx, located = grid_forward_ref(T(x), T(table), off, res, torch.float64)
        o_out, o_dy = oracle_lib.grid_forward(x, table, off, res, calc_dy_dx=True)
        o_dy = T(o_dy).view(N, L, D, C)
        # the input gradient is a function of (grad, dy_dx): both sides get the oracle's dy_dx
        gt, counts, gi = grid_backward_ref(T(grad), located, off, C, o_dy, torch.float64)
        o_gt, o_gi = oracle_lib.grid_backward(grad, x, table, off, res, o_dy.reshape(N, -1).numpy())
        tmax = torch.stack([T(table[off[l]:off[l + 1]]).abs().max() for l in range(L)]).double()
        s_out = tmax.view(L, 1, 1)
        s_dy = (tmax * (T(np.asarray(res)).double() - 2)).view(1, L, 1, 1)
        worst["out"] = max(worst["out"], err(T(o_out), out, s_out))
        worst["dy_dx"] = max(worst["dy_dx"], err(o_dy, dy_dx, s_dy))
        if float(gt.abs().max()) > 0:
            worst["table"] = max(worst["table"], err(T(o_gt), gt, float(gt.abs().max())))
        if float(gi.abs().max()) > 0:
            worst["inputs"] = max(worst["inputs"], err(T(o_gi), gi, float(gi.abs().max())))
        assert bool((T(o_gt)[counts == 0] == 0).all()) and bool((gt[counts == 0] == 0).all())
        outside = ((T(x) < 0) | (T(x) > 1)).any(1)
        assert int(outside.sum()) == min(max(N - 2, 0), 2)
        for t in (out[:, outside], T(o_out)[:, outside], dy_dx[outside], o_dy[outside], gi[outside], T(o_gi)[outside]):
            assert not t.any()
        for l in range(L):
            assert not located[l]["valid"][outside].any()
            if res[l] == 2:
                assert not located[l]["valid"].any() and not out[l].any() and not o_out[l].any() and not dy_dx[:, l].any()
                assert not o_dy[:, l].any() and not gt[off[l]:off[l + 1]].any() and not o_gt[off[l]:off[l + 1]].any()
    if PRINT:
        print(f"GRID_REF oracle N={N}: " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert worst["out"] <= 4 * EPS32 and worst["dy_dx"] <= 4 * EPS32 and worst["inputs"] <= 4 * EPS32 and worst["table"] <= 8 * EPS32


def test_row_indices_by_hand():
    """Three cells worked out with Python integers (M = 2^32):
      dense, 3-D, resolution 18, 5832 rows, p = (3, 7, 11):   strides 1, 18, 324 -> 3 + 7 * 18 + 11 * 324 = 3693
      hashed, 3-D, resolution 34, 8192 rows, p = (5, 17, 29): stride 34^3 > 8192; 17 * 2654435761 % M = 2175734977,
          29 * 805459861 % M = 1883499489, 5 ^ 2175734977 ^ 1883499489 = 4058840869, % 8192 = 7973
      hashed, 3-D, resolution 40, 1000 rows, p = (9, 21, 33): 9 ^ (21 * 2654435761 % M) ^ (33 * 805459861 % M) = 3401691577,
          % 1000 = 577 (a power-of-two mask of 1023 would give 3401691577 & 1023 = 441)
      hashed, 2-D, resolution 258, 65536 rows, p = (100, 200): 100 ^ (200 * 2654435761 % M) = 2606174764, % 65536 = 4652
    and the same through grid_forward_ref's corner rows: the point at the centre of the cell p has p as its corner 0."""
    assert 17 * 2654435761 % 2 ** 32 == 2175734977 and 29 * 805459861 % 2 ** 32 == 1883499489
    assert (5 ^ 2175734977 ^ 1883499489) == 4058840869 and 3401691577 & 1023 == 441
    cases = [((3, 7, 11), 18, 5832, 3693), ((5, 17, 29), 34, 8192, 7973), ((9, 21, 33), 40, 1000, 577), ((100, 200), 258, 65536, 4652)]
    for p, res, rows, want in cases:
        assert int(grid_rows(torch.tensor([p], dtype=torch.int64), res, rows)[0]) == want
        x = ((torch.tensor([p], dtype=torch.float64)) / (res - 2)).float()         # pos = p + 0.5 up to rounding
        cell, frac = grid_cells(x, res)
        assert cell[0].tolist() == list(p) and bool(((frac > 0.49) & (frac < 0.51)).all())
        table = torch.arange(rows + 8, dtype=torch.float32).view(-1, 1)
        out, _, located = grid_forward_ref(x, table, [8, rows + 8], [res], torch.float64)
        assert int(located[0]["rows"][0, 0]) == want and bool(located[0]["valid"].all())
        # the far corner, for the upper-neighbour convention: bit d of the corner index moves dimension d
        far = torch.tensor([[c + 1 for c in p]], dtype=torch.int64)
        assert int(located[0]["rows"][0, -1]) == int(grid_rows(far, res, rows)[0])
        one = torch.tensor([[p[0] + 1] + list(p[1:])], dtype=torch.int64)
        assert int(located[0]["rows"][0, 1]) == int(grid_rows(one, res, rows)[0])
        # the level's first row is row offsets[0] of the table: the interpolated "feature" is the mean of the corners' row numbers
        assert abs(float(out[0, 0, 0]) - 8 - float(located[0]["rows"][0].double().mean())) < 1e-3 * rows


@pytest.mark.parametrize("D,C,res,off", [(3, 4, (6, 9, 14), None), (2, 2, (10, 18), None), (3, 2, (40, 57), [0, 1000, 2000]), (1, 1, (16, 64), None)])
def test_scatter_is_the_adjoint_of_the_gather_and_dy_dx_the_derivative(D, C, res, off):
    """An independent float64 statement of the forward (gather the corner rows, multiply by the weights, add) has the statement's
    features; the autograd gradient of its table is grid_backward_ref's scatter-add to 1e-12 of the largest entry.  On points whose
    2^D corners are all interior the renormalisation divides by 1, and (res - 2) times the derivative of the plain multilinear
    interpolation with respect to the fractional position is dy_dx."""
    off = off if off is not None else _levels(D, res, {3: 9, 2: 8, 1: 5}[D])
    N, L = 400, len(res)
    x, table, grad = (T(a) for a in grid_case(D, C, off, res, N, 7))
    out, dy_dx, located = grid_forward_ref(x, table, off, res, torch.float64)
    gt, counts, _ = grid_backward_ref(grad, located, off, C, None, torch.float64)
    tab = table.double().requires_grad_(True)
    gathered = torch.stack([(tab[off[l] + located[l]["rows"]] * (located[l]["w"] * located[l]["valid"])[:, :, None]).sum(1) for l in range(L)])
    assert err(gathered.detach(), out, 1.0) <= 1e-14
    (auto,) = torch.autograd.grad((gathered * grad.double()).sum(), tab)
    assert err(gt, auto, float(auto.abs().max())) <= 1e-12
    assert int(counts.sum()) == sum(int(loc["valid"].sum()) for loc in located)
    for l, r in enumerate(res):
        inside = located[l]["valid"].all(dim=1)
        assert int(inside.sum()) > N // 4
        cell, frac = grid_cells(x, r)
        f = frac.double().requires_grad_(True)
        plain = torch.zeros(N, C, dtype=torch.float64)
        for idx in range(1 << D):
            w = torch.ones(N, dtype=torch.float64)
            for d in range(D):
                w = w * (f[:, d] if (idx >> d) & 1 else 1 - f[:, d])
            plain = plain + w[:, None] * tab.detach()[off[l] + located[l]["rows"][:, idx]]
        assert err(plain[inside].detach(), out[l][inside], 1.0) <= 1e-13
        for c in range(C):
            (d_f,) = torch.autograd.grad(plain[:, c].sum(), f, retain_graph=True)
            assert err((r - 2) * d_f[inside], dy_dx[inside, l, :, c], float(r - 2)) <= 1e-12
