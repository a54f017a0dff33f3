"""NumPy restatement of the dense optical-flow estimator of gsvc_amd.flow (csrc/flow.hip; the algorithm: include/gsvc_hip.h), stage by
stage and whole, the seeded texture the tests run on, their shapes, and the bound the GPU tests hold the kernels to.

Coarse-to-fine Horn-Schunck with warping.  ``dtype`` is the type every stage computes in: float64 is the reference, float32 is what
the bound below was measured on.  Convention: ``flow[0]`` = x displacement, ``flow[1]`` = y displacement in pixels, at the pixel of
frame t, with ``I_t(x, y) ~ I_{t+1}(x + flow[0], y + flow[1])``.
"""
import functools

import numpy as np

DEFAULTS = dict(alpha=0.02, warps=5, iters=30, min_side=8, max_levels=6, max_step=1.0)

# the solver's tile (csrc/flow.hip: FL_EXT cells a side staged per workgroup, FL_K sweeps per launch, FL_EXT - 2 FL_K owned)
SOLVER_EXT, SOLVER_K = 64, 4
SOLVER_OWN = SOLVER_EXT - 2 * SOLVER_K

# 18 x 34: inside one tile.  37 x 53: odd both ways (the pool drops a row and a column, the upsampling clamps).  131 x 139: two
# full tiles of 56 owned cells plus a partial one (19 rows, 27 columns) in each axis.  120 x 136: tiled again, and rows of a multiple
# of four cells: the solver then moves its strips as 16 bytes (its other path).
SHAPES = ((18, 34), (37, 53), (2 * SOLVER_OWN + 19, 2 * SOLVER_OWN + 27), (2 * SOLVER_OWN + 8, 2 * SOLVER_OWN + 24))
TABLE_SHAPES = ((96, 160), (37, 53), (18, 34))
SHIFTS = ((3.3, -1.7), (7.5, 4.2))


# ---- stages ----------------------------------------------------------------------------------------------------------------------
def _shift(a, dy, dx):
    """a[..., clamp(y + dy), clamp(x + dx)]: replicated borders."""
    h, w = a.shape[-2:]
    ys = np.clip(np.arange(h) + dy, 0, h - 1)
    xs = np.clip(np.arange(w) + dx, 0, w - 1)
    return a[..., ys[:, None], xs[None, :]]


def blur(a):
    """Separable 5-tap binomial [1, 4, 6, 4, 1] / 16, vertical then horizontal, replicated borders."""
    dt = a.dtype.type
    v = ((_shift(a, -2, 0) + _shift(a, 2, 0)) + dt(4) * (_shift(a, -1, 0) + _shift(a, 1, 0)) + dt(6) * a) * dt(0.0625)
    return ((_shift(v, 0, -2) + _shift(v, 0, 2)) + dt(4) * (_shift(v, 0, -1) + _shift(v, 0, 1)) + dt(6) * v) * dt(0.0625)


def pool(a):
    """2 x 2 mean; an odd last row or column is dropped."""
    h, w = a.shape[-2] // 2 * 2, a.shape[-1] // 2 * 2
    a = a[..., :h, :w]
    return ((a[..., 0::2, 0::2] + a[..., 0::2, 1::2]) + (a[..., 1::2, 0::2] + a[..., 1::2, 1::2])) * a.dtype.type(0.25)


def level_sizes(H, W, min_side=8, max_levels=6):
    out = [(H, W)]
    while min(out[-1]) // 2 >= min_side and len(out) < max_levels:
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


def pyramid(luma, min_side=8, max_levels=6):
    P = [blur(luma)]
    for _ in level_sizes(*luma.shape[-2:], min_side, max_levels)[1:]:
        P.append(blur(pool(P[-1])))
    return P


def bilinear(a, x, y):
    """a [h, w] at the positions x, y (arrays of one shape), clamped to the picture."""
    dt = a.dtype.type
    h, w = a.shape
    x = np.clip(x, dt(0), dt(w - 1))
    y = np.clip(y, dt(0), dt(h - 1))
    x0 = np.minimum(np.floor(x), dt(w - 2))
    y0 = np.minimum(np.floor(y), dt(h - 2))
    fx, fy = x - x0, y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    a00, a01, a10, a11 = a[y0, x0], a[y0, x0 + 1], a[y0 + 1, x0], a[y0 + 1, x0 + 1]
    top = a00 + fx * (a01 - a00)
    bot = a10 + fx * (a11 - a10)
    return top + fy * (bot - top)


def _grid(h, w, dt):
    ys, xs = np.meshgrid(np.arange(h, dtype=dt), np.arange(w, dtype=dt), indexing="ij")
    return xs, ys


def upsample(coarse, H, W):
    """One flow component from the level below: 2 x bilinear(coarse, (x + 0.5) / 2 - 0.5, (y + 0.5) / 2 - 0.5)."""
    dt = coarse.dtype.type
    xs, ys = _grid(H, W, coarse.dtype)
    return dt(2) * bilinear(coarse, (xs + dt(0.5)) * dt(0.5) - dt(0.5), (ys + dt(0.5)) * dt(0.5) - dt(0.5))


def warp_coefficients(P0, P1, u0, v0):
    """(Ix, Iy, c) of one warp."""
    dt = P0.dtype.type
    h, w = P0.shape
    xs, ys = _grid(h, w, P0.dtype)
    px, py = xs + u0, ys + v0
    Bw = bilinear(P1, px, py)
    half = dt(0.5)
    gx = lambda a: half * (_shift(a, 0, 1) - _shift(a, 0, -1))          # noqa: E731
    gy = lambda a: half * (_shift(a, 1, 0) - _shift(a, -1, 0))          # noqa: E731
    ox = np.maximum(np.maximum(-px, px - dt(w - 1)), dt(0))
    oy = np.maximum(np.maximum(-py, py - dt(h - 1)), dt(0))
    m = np.clip(dt(1) - np.maximum(ox, oy), dt(0), dt(1))
    Ix = m * (half * (gx(P0) + gx(Bw)))
    Iy = m * (half * (gy(P0) + gy(Bw)))
    It = m * (Bw - P0)
    c = (It - Ix * u0) - Iy * v0
    return Ix, Iy, c


def solve(U, V, Ix, Iy, c, alpha, iters):
    """``iters`` Jacobi sweeps: every pixel from the previous iterate."""
    dt = U.dtype.type
    den = dt(1) / ((dt(alpha) * dt(alpha) + Ix * Ix) + Iy * Iy)
    q = dt(0.25)
    for _ in range(iters):
        Ub = q * ((_shift(U, 0, -1) + _shift(U, 0, 1)) + (_shift(U, -1, 0) + _shift(U, 1, 0)))
        Vb = q * ((_shift(V, 0, -1) + _shift(V, 0, 1)) + (_shift(V, -1, 0) + _shift(V, 1, 0)))
        t = ((Ix * Ub + Iy * Vb) + c) * den
        U, V = Ub - Ix * t, Vb - Iy * t
    return U, V


def update(u0, U, max_step):
    dt = u0.dtype.type
    return u0 + np.clip(U - u0, dt(-max_step), dt(max_step))


# ---- whole -----------------------------------------------------------------------------------------------------------------------
def estimate(l0, l1, dtype=np.float64, alpha=0.02, warps=5, iters=30, min_side=8, max_levels=6, max_step=1.0):
    """Two luma planes [H, W] -> flow [2, H, W] in ``dtype``."""
    l0, l1 = np.asarray(l0).astype(dtype), np.asarray(l1).astype(dtype)
    P0, P1 = pyramid(l0, min_side, max_levels), pyramid(l1, min_side, max_levels)
    u = v = None
    for lv in range(len(P0) - 1, -1, -1):
        h, w = P0[lv].shape
        if u is None:
            u, v = np.zeros((h, w), dtype), np.zeros((h, w), dtype)
        else:
            u, v = upsample(u, h, w), upsample(v, h, w)
        for _ in range(warps):
            Ix, Iy, c = warp_coefficients(P0[lv], P1[lv], u, v)
            U, V = solve(u, v, Ix, Iy, c, alpha, iters)
            u, v = update(u, U, max_step), update(v, V, max_step)
    return np.stack([u, v])


def luma_of(rgb):
    """[3, H, W] -> [H, W]: 0.2126 R + 0.7152 G + 0.0722 B."""
    return 0.2126 * rgb[0] + 0.7152 * rgb[1] + 0.0722 * rgb[2]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _texture_terms():
    rng = np.random.default_rng(7)
    fx, fy = rng.uniform(-0.25, 0.25, (2, 24))
    ph = rng.uniform(0, 2 * np.pi, 24)
    am = rng.uniform(0.2, 1, 24)
    return fx, fy, ph, am


def texture(x, y):
    """0.5 + 0.5 sum_k am_k sin(fx_k x + fy_k y + ph_k) / sum am, 24 seeded sinusoids (float64)."""
    fx, fy, ph, am = _texture_terms()
    x, y = np.asarray(x, np.float64)[..., None], np.asarray(y, np.float64)[..., None]
    return 0.5 + 0.5 * (am * np.sin(fx * x + fy * y + ph)).sum(-1) / am.sum()


@functools.lru_cache(maxsize=None)
def texture_pair(H, W, dx, dy):
    """Frame t and frame t + 1 = the texture evaluated at (x - dx, y - dy): float32 [H, W] each (what the kernels are given)."""
    xs, ys = _grid(H, W, np.float64)
    a, b = texture(xs, ys).astype(np.float32), texture(xs - dx, ys - dy).astype(np.float32)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def cube_pair():
    """Luma of frames 2 and 3 of ``SyntheticFrameCube(96, 160, 8, blobs=12)`` (float32 [96, 160]) and the cube's analytic flow."""
    from gsvc_amd.frame import SyntheticFrameCube
    cube = SyntheticFrameCube(96, 160, 8, blobs=12)
    f = [luma_of(cube._image(t)).numpy().astype(np.float32) for t in (2, 3)]
    return f[0], f[1], cube.get_optical_flow(2).numpy()


# the whole-estimate cases of the GPU test: every shape with both shifts, then the cube pair
CASES = tuple((H, W, dx, dy) for (H, W) in SHAPES for (dx, dy) in SHIFTS) + ("cube",)


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    if case == "cube":
        return cube_pair()[:2]
    return texture_pair(*case)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The float64 estimate of a case with the defaults (computed once per test session, shared, read-only)."""
    a, b = case_inputs(case)
    out = estimate(a, b, np.float64)
    out.setflags(write=False)
    return out


def epe(flow, dx, dy):
    """Mean endpoint error in pixels over ALL pixels against a constant shift."""
    return float(np.sqrt((flow[0] - dx) ** 2 + (flow[1] - dy) ** 2).mean())


# ---- the bound of the whole estimate ---------------------------------------------------------------------------------------------
# max |estimate(float32) - estimate(float64)| in pixels over both components and all pixels, measured with this file on CASES
# (tools/bench_flow.py --f32-error prints them):
F32_ERRORS = {(18, 34, 3.3, -1.7): 3.73e-6, (18, 34, 7.5, 4.2): 3.24e-6, (37, 53, 3.3, -1.7): 5.02e-6, (37, 53, 7.5, 4.2): 1.546e-4,
              (131, 139, 3.3, -1.7): 8.32e-6, (131, 139, 7.5, 4.2): 6.27e-6, (120, 136, 3.3, -1.7): 5.60e-6, (120, 136, 7.5, 4.2): 5.61e-6,
              "cube": 1.05e-5}
# (37 x 53 at the larger shift: the ten largest differences, 4e-5 .. 1.5e-4, lie in the first rows of the picture, where the warped
# position leaves it and the outside ramp acts; the median difference of that case is 8e-7)
F32_ERROR = max(F32_ERRORS.values())
# 4 x the largest: the margin covers FMA contraction, a hardware reciprocal and another summation order in the blur; never above
# 1e-3 px (a wrong stencil or halo shows up orders of magnitude above that)
ESTIMATE_BOUND = min(4 * F32_ERROR, 1e-3)
# one pyramid step: values of order 1, two passes of five taps: a few float32 ulps of 1
PYRAMID_BOUND = 4 * 2.0 ** -23
