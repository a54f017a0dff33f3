"""Plain NumPy statements of DESIGN.md "Raster spec" for the direct tests of the rasterizer kernels.

Written from the spec, not from the kernels; every function takes ``dtype``: float64 is the reference, float32 the same statement
at the kernels' precision (its distance from the float64 run is the ``e32`` of the rule ``e_kernel <= 4 e32 + 4 eps32``).

  preprocess_ref       spec steps 1-4 per Gaussian: u, v, depth, conic, 2-D covariance
  blend_ref            spec step 6 over given tile lists, ``form`` = "literal" (power from (dx, dy)) or "poly" (log2(alpha) as a
                       polynomial about the 8x8 quadrant centre); per-(pixel, entry) decisions out and, for another dtype, in
  blend_bwd_rows_ref   spec step 7 per (tile, Gaussian) instance: the nine (ten) sums and the sums of their absolute terms
  gaussian_bwd_ref     one Gaussian's totals -> the six (seven) gradients; ``mag=True``: the sum of the magnitudes of all terms
  scene                the scenes of tests/test_raster_kernels_gpu.py, built from their seeds (the CPU test asserts their
                       borderline share)

``geom`` is [P, 6+] float: u, v, depth, A, B, C (the first six columns of the oracle's ``geom``).  Lists are the oracle's:
``tile_ranges`` [tiles, 2], ``point_list`` [instances].  ``settings``: dict(H, W, bg, flags, ...) as gsvc_amd.synthetic makes it.
"""
import numpy as np

TILE = 16
ALPHA_MIN = 1.0 / 255.0
ALPHA_MAX = 0.99
T_MIN = 1e-4
LOG2E = 1.4426950408889634
F_PIXEL_CORNER, F_PIXEL_UNITS, F_CLAMP_STOP, F_NO_LOW_PASS = 2, 8, 16, 32
# the oracle's own margins (oracle/raster_oracle.c): a decision this close to its boundary may fall either way
M_POWER, M_ALPHA, M_T = 1e-6, 2e-5 / 255.0, 1e-8


def _c(x, dtype):
    return np.asarray(x, dtype=dtype)


def low_pass_of(settings):
    if int(settings.get("flags", 0)) & F_NO_LOW_PASS:
        return 0.0
    return float(settings.get("low_pass", 0.0)) or 0.3


# ------------------------------------------------------------------------------------------------------------- steps 1-4
def cov3d_ref(scales, rotations, settings, dtype):
    """R S^2 R^T as its six stored numbers [P, 6] = xx xy xz yy yz zz, S = scale_modifier * scales, in the oracle's order of
    operations (in float32: the bits a cov3D_precomp must hold to give the scale / rotation call's results downstream)."""
    f = dtype
    q, s = _c(rotations, f), _c(scales, f)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = f(1.0), f(2.0)
    R = [[one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)],
         [two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)],
         [two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)]]
    sm = f(np.float32(settings.get("scale_modifier", 1.0)))
    S = [sm * s[:, 0], sm * s[:, 1], sm * s[:, 2]]
    L = [[R[a][k] * S[k] for k in range(3)] for a in range(3)]
    c = lambda a, b: L[a][0] * L[b][0] + L[a][1] * L[b][1] + L[a][2] * L[b][2]
    return np.stack([c(0, 0), c(0, 1), c(0, 2), c(1, 1), c(1, 2), c(2, 2)], axis=1)


def preprocess_ref(means3D, scales, rotations, settings, dtype, view="viewmatrix", cov3D=None):
    """u, v, depth, A, B, C, a, b, c (2-D covariance, low-pass included) and det per Gaussian; no culling (steps 1-4 only)."""
    f = dtype
    p = _c(means3D, f)
    M = _c(np.asarray(settings[view], np.float32), f)
    sc, lp = f(np.float32(settings["scale"])), f(np.float32(low_pass_of(settings)))
    x_min, y_min = f(np.float32(settings["x_min"])), f(np.float32(settings["y_min"]))
    off = f(0.0) if int(settings.get("flags", 0)) & F_PIXEL_CORNER else f(0.5)
    xv = M[0, 0] * p[:, 0] + M[0, 1] * p[:, 1] + M[0, 2] * p[:, 2] + M[0, 3]
    yv = M[1, 0] * p[:, 0] + M[1, 1] * p[:, 1] + M[1, 2] * p[:, 2] + M[1, 3]
    zv = M[2, 0] * p[:, 0] + M[2, 1] * p[:, 1] + M[2, 2] * p[:, 2] + M[2, 3]
    cv = _c(cov3D, f) if cov3D is not None else cov3d_ref(scales, rotations, settings, f)
    C3 = [[cv[:, 0], cv[:, 1], cv[:, 2]], [cv[:, 1], cv[:, 3], cv[:, 4]], [cv[:, 2], cv[:, 4], cv[:, 5]]]
    T0 = [sc * M[0, 0], sc * M[0, 1], sc * M[0, 2]]
    T1 = [sc * M[1, 0], sc * M[1, 1], sc * M[1, 2]]
    U0 = [C3[a][0] * T0[0] + C3[a][1] * T0[1] + C3[a][2] * T0[2] for a in range(3)]
    U1 = [C3[a][0] * T1[0] + C3[a][1] * T1[1] + C3[a][2] * T1[2] for a in range(3)]
    ca = T0[0] * U0[0] + T0[1] * U0[1] + T0[2] * U0[2] + lp
    cb = T0[0] * U1[0] + T0[1] * U1[1] + T0[2] * U1[2]
    cc = T1[0] * U1[0] + T1[1] * U1[1] + T1[2] * U1[2] + lp
    det = ca * cc - cb * cb
    with np.errstate(divide="ignore", invalid="ignore"):
        det_inv = f(1.0) / det
    u = (xv - x_min) * sc - off
    v = (yv - y_min) * sc - off
    return dict(u=u, v=v, depth=zv, A=cc * det_inv, B=-cb * det_inv, C=ca * det_inv, a=ca, b=cb, c=cc, det=det)


# ---------------------------------------------------------------------------------------------------------------- step 6
def _tile_pixels(t, gx, H, W):
    tx, ty = t % gx, t // gx
    ly, lx = np.divmod(np.arange(TILE * TILE), TILE)
    px, py = tx * TILE + lx, ty * TILE + ly
    return tx, ty, px, py, (px < W) & (py < H)


def _log2alpha_poly(g, o, cx, cy, x, y, f):
    """log2(o) - [A'(U-x)^2 + C'(V-y)^2 + B'(U-x)(V-y)] as the polynomial n0 + n1 x + n2 y + n3 x^2 + n4 y^2 + n5 xy in the pixel's
    offset (x, y) from the centre (cx, cy); U = u - cx, V = v - cy; A' = A log2(e)/2, B' = B log2(e), C' = C log2(e)/2.  The sum
    is taken in the order n0 + n5 xy, + n1 x, + n2 y, + n3 x^2, + n4 y^2 (blend_pass's header and alpha_of)."""
    Ap, Bp, Cp = f(0.5 * LOG2E) * g[3], f(LOG2E) * g[4], f(0.5 * LOG2E) * g[5]
    U, V = g[0] - cx, g[1] - cy
    n0 = np.log2(o) - (Ap * U * U + Cp * V * V + Bp * U * V)
    n1, n2 = f(2.0) * Ap * U + Bp * V, f(2.0) * Cp * V + Bp * U
    t = (-Bp) * (x * y) + n0
    t = n1 * x + t
    t = n2 * y + t
    t = (-Ap) * (x * x) + t
    t = (-Cp) * (y * y) + t
    return t


def _raw_alpha(g, o, px, py, f, form, centre):
    """(power <= 0 test input, o G, G) of one entry at the tile's pixels.  literal: power from (dx, dy) as the oracle does;
    poly: about ``centre`` = (cx[256], cy[256]); G = oG / o there and no power test (the form serves positive definite conics)."""
    if form == "literal":
        dx, dy = g[0] - px.astype(f), g[1] - py.astype(f)
        power = f(-0.5) * (g[3] * dx * dx + g[5] * dy * dy) - g[4] * dx * dy
        G = np.exp(np.minimum(power, f(0.0)))
        return power, o * G, G
    cx, cy = centre
    t = _log2alpha_poly(g, o, cx, cy, px.astype(f) - cx, py.astype(f) - cy, f)
    oG = np.exp2(t)
    return np.full(px.shape, f(-1.0)), oG, oG / o


def blend_ref(geom, opacities, colours, tile_ranges, point_list, settings, dtype, form="literal", decisions=None, maps=False):
    """Spec step 6 over the given lists.  Returns dict(image [3,H,W], final_T, n_contrib, depth, alpha (maps=True), image_scale
    and depth_scale (the sums of the absolute terms: sum |c| w + T |bg|, sum w |z|), decisions
    {tile: (contrib [n,256] bool, clamp [n,256] bool)}, borderline [H,W] bool: the oracle's margins on this run's numbers)."""
    f = dtype
    H, W = int(settings["H"]), int(settings["W"])
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    geom, op, col = _c(geom, f), _c(opacities, f).reshape(-1), _c(colours, f)
    bg = _c(np.asarray(settings.get("bg", (0, 0, 0)), np.float32), f)
    nch = 5 if maps else 3
    out = np.zeros((nch, H, W), f)
    final_T, n_contrib = np.ones((H, W), f), np.zeros((H, W), np.int32)
    border = np.zeros((H, W), bool)
    scale = np.zeros((4, H, W), np.float64)
    dec_out = {}
    for t in range(gx * gy):
        s0, s1 = int(tile_ranges[t][0]), int(tile_ranges[t][1])
        tx, ty, px, py, inside = _tile_pixels(t, gx, H, W)
        centre = (((px // 8) * 8 + 3.5).astype(f), ((py // 8) * 8 + 3.5).astype(f))
        T = np.ones(256, f)
        C = np.zeros((nch, 256), f)
        Cs = np.zeros((4, 256), np.float64)            # sums of the absolute terms: three channels and the depth map
        last = np.zeros(256, np.int32)
        done = ~inside
        bl = np.zeros(256, bool)
        n = s1 - s0
        contrib_t, clamp_t = np.zeros((n, 256), bool), np.zeros((n, 256), bool)
        for j in range(n):
            i = int(point_list[s0 + j])
            g, o = geom[i], op[i]
            power, oG, _ = _raw_alpha(g, o, px, py, f, form, centre)
            alpha = np.minimum(f(ALPHA_MAX), oG)
            test_T = T * (f(1.0) - alpha)
            if decisions is None:
                pos = power > 0
                small = alpha < f(ALPHA_MIN)
                cand = ~done & ~pos & ~small
                stop = cand & (test_T < f(T_MIN))
                contrib = cand & ~stop
                clamp = oG > f(ALPHA_MAX)
                live = ~done
                bl |= live & (np.abs(power) < M_POWER) if form == "literal" else False
                bl |= live & ~pos & (np.abs(alpha - f(ALPHA_MIN)) < M_ALPHA)
                bl |= cand & (np.abs(test_T - f(T_MIN)) < M_T)
                bl |= cand & (np.abs(oG - f(ALPHA_MAX)) < 2e-5 * ALPHA_MAX)       # (the clamp's own boundary, same kind of margin)
                done = done | stop
            else:
                contrib, clamp = decisions[t][0][j], decisions[t][1][j]
                alpha = np.where(clamp, f(ALPHA_MAX), oG)
                test_T = T * (f(1.0) - alpha)
            contrib_t[j], clamp_t[j] = contrib, clamp & contrib
            w = np.where(contrib, alpha * T, f(0.0))
            C[0] += col[i, 0] * w
            C[1] += col[i, 1] * w
            C[2] += col[i, 2] * w
            if maps:
                C[3] += g[2] * w
            Cs += np.abs(np.array([col[i, 0], col[i, 1], col[i, 2], g[2]], np.float64))[:, None] * w.astype(np.float64)
            T = np.where(contrib, test_T, T)
            last = np.where(contrib, j + 1, last)
        dec_out[t] = (contrib_t, clamp_t)
        ok = inside
        out[0, py[ok], px[ok]] = (C[0] + T * bg[0])[ok]
        out[1, py[ok], px[ok]] = (C[1] + T * bg[1])[ok]
        out[2, py[ok], px[ok]] = (C[2] + T * bg[2])[ok]
        if maps:
            out[3, py[ok], px[ok]] = C[3][ok]
            out[4, py[ok], px[ok]] = (f(1.0) - T)[ok]
        scale[:3, py[ok], px[ok]] = (Cs[:3] + T.astype(np.float64) * np.abs(bg.astype(np.float64))[:, None])[:, ok]
        scale[3, py[ok], px[ok]] = Cs[3][ok]
        final_T[py[ok], px[ok]] = T[ok]
        n_contrib[py[ok], px[ok]] = last[ok]
        border[py[ok], px[ok]] = bl[ok]
    r = dict(image=out[:3], final_T=final_T, n_contrib=n_contrib, decisions=dec_out, borderline=border, image_scale=scale[:3],
             depth_scale=scale[3])
    if maps:
        r["depth"], r["alpha"] = out[3], out[4]
    return r


def decisions_differ(a, b, H, W):
    """[H, W] bool: pixels where two runs' decision masks differ anywhere."""
    gx = (W + TILE - 1) // TILE
    d = np.zeros((H, W), bool)
    for t in a:
        _, _, px, py, inside = _tile_pixels(t, gx, H, W)
        diff = ((a[t][0] != b[t][0]) | (a[t][1] != b[t][1])).any(axis=0) & inside
        d[py[diff], px[diff]] = True
    return d


def forward_refs(geom, opacities, colours, tile_ranges, point_list, settings, oracle_borderline=None, maps=False, forms=("literal", "poly")):
    """The float64 run (literal), the float32 runs of ``forms`` with the float64 decisions (pure arithmetic) and the borderline
    mask of the issue: the float64 run's margins | a float32 form deciding for itself decides differently | the oracle's mark."""
    H, W = int(settings["H"]), int(settings["W"])
    args = (geom, opacities, colours, tile_ranges, point_list, settings)
    r64 = blend_ref(*args, np.float64, "literal", maps=maps)
    border = r64["borderline"].copy()
    r32 = {}
    for form in forms:
        own = blend_ref(*args, np.float32, form)
        border |= own["borderline"] | decisions_differ(own["decisions"], r64["decisions"], H, W)
        r32[form] = blend_ref(*args, np.float32, form, decisions=r64["decisions"], maps=maps)
    if oracle_borderline is not None:
        border |= np.asarray(oracle_borderline) != 0
    return r64, r32, border


# ---------------------------------------------------------------------------------------------------------------- step 7
def blend_bwd_rows_ref(geom, opacities, colours, tile_ranges, point_list, settings, final_T, decisions, dL_dimage, dtype,
                       form="literal", dL_ddepth=None, dL_dalpha=None, shift_mags=None):
    """The back-to-front recurrence of spec step 7.  ``decisions``: blend_ref's (who contributed where, where the clamp was
    active); ``final_T`` [H, W] the forward's.  Returns (rows [instances, 9 | 10], mags the same shape): per list position the sums
    over the tile's pixels of h, h dx, h dy, h dx^2, h dx dy, h dy^2, w d_r, w d_g, w d_b (, w gD) with h = G dL/dalpha, dx = u - px,
    and the sums of the absolute values of the same terms.  form="poly": log2(alpha) as the polynomial about the TILE centre,
    moments of o h about the tile centre, then shifted to the Gaussian's centre and divided by o (k_blend_bwd_tile's flush);
    ``shift_mags`` [instances, 6], when given, receives the size of what that shift adds up before it cancels."""
    f = dtype
    H, W = int(settings["H"]), int(settings["W"])
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    clamp_stop = bool(int(settings.get("flags", 0)) & F_CLAMP_STOP)
    geom, op, col = _c(geom, f), _c(opacities, f).reshape(-1), _c(colours, f)
    bg = _c(np.asarray(settings.get("bg", (0, 0, 0)), np.float32), f)
    aux = dL_ddepth is not None or dL_dalpha is not None
    ns = 10 if aux else 9
    n_inst = int(np.max(np.asarray(tile_ranges)[:, 1])) if len(tile_ranges) else 0
    rows, mags = np.zeros((n_inst, ns), f), np.zeros((n_inst, ns), np.float64)
    dL = _c(dL_dimage, f)
    gDm = _c(dL_ddepth, f) if dL_ddepth is not None else np.zeros((H, W), f)
    gAm = _c(dL_dalpha, f) if dL_dalpha is not None else np.zeros((H, W), f)
    Tfm = _c(final_T, f)
    for t in range(gx * gy):
        s0, s1 = int(tile_ranges[t][0]), int(tile_ranges[t][1])
        if s1 == s0:
            continue
        tx, ty, px, py, inside = _tile_pixels(t, gx, H, W)
        pxc, pyc = np.minimum(px, W - 1), np.minimum(py, H - 1)
        d = np.where(inside, dL[:, pyc, pxc], f(0.0))
        gD, gA = np.where(inside, gDm[pyc, pxc], f(0.0)), np.where(inside, gAm[pyc, pxc], f(0.0))
        Tf = np.where(inside, Tfm[pyc, pxc], f(1.0))
        tb = Tf * (bg[0] * d[0] + bg[1] * d[1] + bg[2] * d[2])
        T = Tf.copy()
        bd = np.zeros(256, f)
        tcx, tcy = f(tx * TILE + 7.5), f(ty * TILE + 7.5)
        x, y = px.astype(f) - tcx, py.astype(f) - tcy
        contrib_t, clamp_t = decisions[t]
        for j in range(s1 - s0 - 1, -1, -1):
            valid = contrib_t[j]
            if not valid.any():
                continue
            i = int(point_list[s0 + j])
            g, o = geom[i], op[i]
            dx, dy = g[0] - px.astype(f), g[1] - py.astype(f)
            _, oG, G = _raw_alpha(g, o, px, py, f, form, (np.full(256, tcx), np.full(256, tcy)))
            alpha = np.where(valid, np.where(clamp_t[j], f(ALPHA_MAX), oG), f(0.0))
            live = valid & ~clamp_t[j] if clamp_stop else valid
            cd = col[i, 0] * d[0] + col[i, 1] * d[1] + col[i, 2] * d[2]
            if aux:
                cd = cd + g[2] * gD + gA
            oma = f(1.0) - alpha
            T = T / oma
            w = alpha * T
            dLda = (cd - bd) * T - tb / oma
            bd = alpha * cd + oma * bd
            k = s0 + j
            wd = [w * d[0], w * d[1], w * d[2]] + ([w * gD] if aux else [])
            if form == "literal":
                h = np.where(live, G, f(0.0)) * dLda
                terms = [h, h * dx, h * dy, h * dx * dx, h * dx * dy, h * dy * dy]
                rows[k, :6] = [np.sum(v, dtype=f) for v in terms]
            else:
                hp = np.where(live, oG, f(0.0)) * dLda                       # o h
                m0, mx, my, mxx, mxy, myy = [np.sum(v, dtype=f) for v in (hp, hp * x, hp * y, hp * (x * x), hp * (x * y), hp * (y * y))]
                U, V, io = g[0] - tcx, g[1] - tcy, f(1.0) / o
                rows[k, :6] = [m0 * io, (U * m0 - mx) * io, (V * m0 - my) * io, (U * (U * m0 - f(2.0) * mx) + mxx) * io,
                               ((U * (V * m0 - my) + mxy) - V * mx) * io, (V * (V * m0 - f(2.0) * my) + myy) * io]
                h = hp * io
                if shift_mags is not None:
                    # what the shift adds up before it cancels: |h| (|U| + |x|)^a (|V| + |y|)^b >= the magnitudes of the terms of
                    # U^2 m0 - 2 U mx + mxx and its five siblings
                    ah, ax, ay = np.abs(h.astype(np.float64)), np.abs(float(U)) + np.abs(x), np.abs(float(V)) + np.abs(y)
                    shift_mags[k] = [np.sum(ah), np.sum(ah * ax), np.sum(ah * ay), np.sum(ah * ax * ax), np.sum(ah * ax * ay),
                                     np.sum(ah * ay * ay)]
                terms = [h, h * dx, h * dy, h * dx * dx, h * dx * dy, h * dy * dy]
            rows[k, 6:] = [np.sum(v, dtype=f) for v in wd]
            mags[k] = [np.sum(np.abs(v.astype(np.float64))) for v in terms + wd]
    return rows, mags


def sum_rows_per_gaussian(rows, point_list, P, dtype=np.float64):
    """A Gaussian's rows added in list (= tile) order."""
    out = np.zeros((P, rows.shape[1]), dtype)
    pl = np.asarray(point_list[: rows.shape[0]], np.int64)
    if dtype == np.float64:
        np.add.at(out, pl, rows.astype(np.float64))
    else:
        for k in range(rows.shape[0]):
            out[pl[k]] += rows[k].astype(dtype)
    return out


class _Mag:
    """A non-negative number standing for the sum of the magnitudes of an expression's terms: + and - add, * multiplies."""

    def __init__(self, v):
        self.v = np.abs(np.asarray(v.v if isinstance(v, _Mag) else v, np.float64))

    def __add__(self, o):
        return _Mag(self.v + _Mag(o).v)

    __radd__ = __sub__ = __rsub__ = __add__

    def __mul__(self, o):
        return _Mag(self.v * _Mag(o).v)

    __rmul__ = __mul__

    def __neg__(self):
        return self


def gaussian_bwd_ref(row_sums, inputs, settings, dtype, mag=False, view="viewmatrix"):
    """One Gaussian's nine (ten) totals -> dL/d(means2D, means3D, colors, opacities, scales | cov3D, rotations) as the spec's step 7 and
    the oracle's formulas have it.  ``inputs``: dict(means3D, scales, rotations, opacities, radii[, cov3D]).  ``mag=True``: every
    product is replaced by its magnitude and every sum by the sum of magnitudes (coefficients that come out of a division — the
    conic, 1 / (det^2 + 1e-7) — enter by their float64 magnitude): the per-element scale of this stage."""
    f = np.float64 if mag else dtype
    wrap = _Mag if mag else (lambda a: a)
    pre = preprocess_ref(inputs["means3D"], inputs.get("scales"), inputs.get("rotations"), settings, f, view, inputs.get("cov3D"))
    s = _c(row_sums, f)
    P = s.shape[0]
    op = wrap(_c(inputs["opacities"], f).reshape(-1))
    A, B, C = wrap(pre["A"]), wrap(pre["B"]), wrap(pre["C"])
    sh, sx, sy, sxx, sxy, syy = (wrap(s[:, k]) for k in range(6))
    M = _c(np.asarray(settings[view], np.float32), f)
    sc = f(np.float32(settings["scale"]))
    flags = int(settings.get("flags", 0))
    H, W = int(settings["H"]), int(settings["W"])
    half, two = f(0.5), f(2.0)
    du = -(op * (A * sx + B * sy))
    dv = -(op * (C * sy + B * sx))
    dA, dB, dC = -(half * op * sxx), -(op * sxy), -(half * op * syy)
    g2 = [du, dv] if flags & F_PIXEL_UNITS else [du * (half * f(W)), dv * (half * f(H))]
    g3 = [sc * (M[0, j] * du + M[1, j] * dv) for j in range(3)]
    if s.shape[1] > 9:
        g3 = [g3[j] + wrap(s[:, 9]) * M[2, j] for j in range(3)]
    ca, cb, cc = wrap(pre["a"]), wrap(pre["b"]), wrap(pre["c"])
    det_true = pre["a"] * pre["c"] - pre["b"] * pre["b"]
    det = wrap(det_true) if not mag else ca * cc + cb * cb
    inv2 = wrap(f(1.0) / (det_true * det_true + f(1e-7)))
    dLa = inv2 * (-(cc * cc * dA) + cb * cc * dB + (det - ca * cc) * dC)
    dLc = inv2 * (-(ca * ca * dC) + ca * cb * dB + (det - ca * cc) * dA)
    dLb = inv2 * (two * cb * cc * dA - (det + two * cb * cb) * dB + two * ca * cb * dC)
    T0, T1 = [sc * M[0, j] for j in range(3)], [sc * M[1, j] for j in range(3)]
    G3 = [[T0[r] * dLa * T0[c] + half * dLb * (T0[r] * T1[c] + T1[r] * T0[c]) + T1[r] * dLc * T1[c] for c in range(3)] for r in range(3)]
    out = {}
    if inputs.get("cov3D") is not None:
        out["cov3D"] = [G3[0][0], G3[0][1] + G3[1][0], G3[0][2] + G3[2][0], G3[1][1], G3[1][2] + G3[2][1], G3[2][2]]
        gs, gq = [wrap(np.zeros(P, f))] * 3, [wrap(np.zeros(P, f))] * 4
    else:
        q = _c(inputs["rotations"], f)
        qr, qx, qy, qz = (wrap(q[:, k]) for k in range(4))
        one = wrap(np.ones(P, f))
        R = [[one - two * (qy * qy + qz * qz), two * (qx * qy - qr * qz), two * (qx * qz + qr * qy)],
             [two * (qx * qy + qr * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - qr * qx)],
             [two * (qx * qz - qr * qy), two * (qy * qz + qr * qx), one - two * (qx * qx + qy * qy)]]
        sm = f(np.float32(settings.get("scale_modifier", 1.0)))
        sv = _c(inputs["scales"], f)
        S = [wrap(sm * sv[:, k]) for k in range(3)]
        dR = [[None] * 3 for _ in range(3)]
        gs = []
        for k in range(3):
            acc = None
            for r in range(3):
                v = two * (G3[r][0] * R[0][k] * S[k] + G3[r][1] * R[1][k] * S[k] + G3[r][2] * R[2][k] * S[k])
                acc = v * R[r][k] if acc is None else acc + v * R[r][k]
                dR[r][k] = v * S[k]
            gs.append(acc * sm)
        gq = [two * (-(qz * dR[0][1]) + qy * dR[0][2] + qz * dR[1][0] - qx * dR[1][2] - qy * dR[2][0] + qx * dR[2][1]),
              two * (qy * dR[0][1] + qz * dR[0][2] + qy * dR[1][0] - two * qx * dR[1][1] - qr * dR[1][2] + qz * dR[2][0] + qr * dR[2][1]
                     - two * qx * dR[2][2]),
              two * (-(two * qy * dR[0][0]) + qx * dR[0][1] + qr * dR[0][2] + qx * dR[1][0] + qz * dR[1][2] - qr * dR[2][0] + qz * dR[2][1]
                     - two * qy * dR[2][2]),
              two * (-(two * qz * dR[0][0]) - qr * dR[0][1] + qx * dR[0][2] + qr * dR[1][0] - two * qz * dR[1][1] + qy * dR[1][2]
                     + qx * dR[2][0] + qy * dR[2][1])]
    val = (lambda e: e.v) if mag else (lambda e: np.asarray(e, f))
    zero = np.zeros(P, f)
    live = (np.asarray(inputs["radii"]) > 0) & (np.asarray(inputs["opacities"]).reshape(-1) > 0)

    def pack(cols):
        a = np.stack([np.broadcast_to(val(c), (P,)) for c in cols], axis=1).astype(f)
        a[~live] = 0
        return a
    out.update(means2D=pack(g2 + [wrap(zero)]), means3D=pack(g3), colors=pack([wrap(s[:, 6]), wrap(s[:, 7]), wrap(s[:, 8])]),
               opacities=pack([sh]), scales=pack(gs), rotations=pack(gq))
    if "cov3D" in out:
        out["cov3D"] = pack(out["cov3D"])
    return out


def unsafe_conic(geom):
    """Per Gaussian: the conic fails the kernels' test for the polynomial form (A, C > 0 and A C >= 1.002 B^2): its chunks take
    the literal loops."""
    g = np.asarray(geom, np.float32)
    A, B, C = g[:, 3], g[:, 4], g[:, 5]
    return ~((A > 0) & (C > 0) & (A * C >= np.float32(1.002) * (B * B)))


GRADS = ("means2D", "means3D", "colors", "opacities", "scales", "rotations")


def rule_errors(got, ref64, scale):
    """|got - ref64| / scale per element; where the scale is zero: 0 if got equals ref64 exactly, else inf; inf for a non-finite got."""
    got, ref64, scale = (np.asarray(a, np.float64) for a in (got, ref64, scale))
    diff = np.abs(got - ref64)
    nz = scale > 0
    e = np.where(nz, diff / np.where(nz, scale, 1.0), np.where(diff == 0, 0.0, np.inf))
    return np.where(np.isfinite(got), e, np.inf)


def rule_error(got, ref64, scale, keep=None):
    """max |got - ref64| / scale per element, over the elements with a non-zero scale (zero scale: got must equal ref64 exactly)."""
    e = rule_errors(got, ref64, scale)
    if keep is not None:
        e = e[keep]
    return float(e.max()) if e.size else 0.0


EPS32 = float(np.finfo(np.float32).eps)


def within_rule(e_kernel, e32):
    return e_kernel <= 4.0 * e32 + 4.0 * EPS32


# ---------------------------------------------------------------------------------------------------------------- scenes
def _stacked(n, seed, clamp):
    """n Gaussians stacked on the tiles of a 32 x 32 image, every one reaching all four quadrants of the tile under its centre.
    Low opacities: nothing stops early.  clamp: high opacities, a few of them 1 (alpha reaches the 0.99 clamp at their centres,
    T < 1e-4 stops the pixels there and leaves entries behind the last contributor)."""
    from gsvc_amd import synthetic
    sc = synthetic.raster_scene(n, H=32, W=32, T=32, seed=seed, window_frames=8, sigma_px=(5.0, 7.0), opacity=(0.02, 0.04))
    s = sc["settings"]
    rng = np.random.default_rng(1000 + seed)
    # centres within 1.5 px of the centre of tile (0, 0): pixel (7.5, 7.5)
    u = 7.5 + rng.uniform(-1.5, 1.5, n)
    v = 7.5 + rng.uniform(-1.5, 1.5, n)
    if clamp:
        sc["opacities"][:] = rng.uniform(0.3, 0.9, (n, 1)).astype(np.float32)
        full = np.argsort(sc["means3D"][:, 2], kind="stable")[::7]      # the nearest and every seventh behind it: opacity 1,
        sc["opacities"][full] = 1.0                                      # a pixel centre 0.36 px from theirs (G = 0.998 > 0.99)
        u[full], v[full] = np.round(u[full]) + 0.3, np.round(v[full]) + 0.2
    sc["means3D"][:, 0] = ((u + 0.5) / s["scale"] + s["x_min"]).astype(np.float32)
    sc["means3D"][:, 1] = ((v + 0.5) / s["scale"] + s["y_min"]).astype(np.float32)
    return sc


def _big(seed):
    """192 x 192 (144 tiles): one Gaussian over >= 129 tiles, one over >= 64, rectangles of 1..5 tiles, and faint Gaussians whose
    alpha box misses tiles of their 3-sigma rectangle."""
    from gsvc_amd import synthetic
    P = 40
    sc = synthetic.raster_scene(P, H=192, W=192, T=64, seed=seed, window_frames=8, sigma_px=(1.0, 3.0), opacity=(0.2, 0.8))
    s = sc["settings"]

    def place(i, u, v, sig, o):
        sc["means3D"][i, 0] = np.float32((u + 0.5) / s["scale"] + s["x_min"])
        sc["means3D"][i, 1] = np.float32((v + 0.5) / s["scale"] + s["y_min"])
        sc["scales"][i] = np.asarray(sig, np.float32) / s["scale"]
        sc["rotations"][i] = (1.0, 0.0, 0.0, 0.0)
        sc["opacities"][i] = o
    place(0, 96.0, 90.0, (34.0, 34.0, 1.0), 0.5)        # radius 103: the whole 12 x 12 grid (144 tiles, two 128-row rounds)
    place(1, 60.0, 70.0, (21.0, 21.0, 1.0), 0.6)        # radius 64: 9 x 9 = 81 tiles (the cooperative sum, one round)
    place(2, 24.3, 23.8, (1.5, 1.5, 1.0), 0.7)          # 1 tile
    place(3, 32.2, 40.1, (1.5, 1.5, 1.0), 0.7)          # 2 tiles
    place(4, 56.0, 104.0, (4.5, 1.0, 1.0), 0.7)         # 3 tiles in a row
    place(5, 128.1, 31.9, (1.5, 1.5, 1.0), 0.7)         # 2 x 2 tiles
    place(6, 152.0, 120.0, (10.0, 1.0, 1.0), 0.7)       # 5 tiles in a row
    for i in range(7, 15):                              # faint and wide: alpha >= 1/255 only near the centre
        place(i, 20.0 + 20.0 * (i - 7), 150.0 + 3.0 * (i - 7), (9.0, 9.0, 1.0), 0.006)
    sc["opacities"][15], sc["opacities"][16] = 0.0, -0.25      # culled by opacity <= 0
    sc["means3D"][17, 2] += 10 * s["threshold"]                 # culled by the slab
    sc["means3D"][18, 0] = 50.0                                 # off screen
    return sc


def _needles(sc, every=64):
    """GSVC_RASTER_NO_LOW_PASS + one near-degenerate conic (A C < 1.002 B^2) per `every` Gaussians: the literal path."""
    s = sc["settings"]
    s["flags"] = int(s.get("flags", 0)) | F_NO_LOW_PASS
    major, minor = 40.0, 0.5
    idx = np.arange(0, sc["means3D"].shape[0], every)
    sc["scales"][idx] = np.array([major, minor, minor], np.float32) / s["scale"]
    c, sn = np.cos(np.pi / 8), np.sin(np.pi / 8)
    sc["rotations"][idx] = np.array([c, 0.0, 0.0, sn], np.float32)
    a, b = (major ** 2 + minor ** 2) * 0.5, (major ** 2 - minor ** 2) * 0.5
    assert a * a < 1.002 * b * b
    return sc


STACK_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 129)
SCENES = {
    "R300": lambda: ("raster", dict(P=300, H=64, W=96, seed=0, sigma_px=(0.5, 6.0))),
    "R400": lambda: ("raster", dict(P=400, H=40, W=56, seed=0, sigma_px=(0.5, 12.0))),
    "R600": lambda: ("raster", dict(P=600, H=48, W=54, seed=3, sigma_px=(0.5, 6.0))),
    "L300": lambda: ("needles", dict(P=300, H=64, W=96, seed=3, sigma_px=(0.5, 6.0))),
    "B": lambda: ("big", dict(seed=4)),
}
for _n in STACK_COUNTS:
    SCENES[f"S{_n}"] = (lambda n=_n: ("stacked", dict(n=n, seed=n, clamp=False)))
    SCENES[f"S{_n}c"] = (lambda n=_n: ("stacked", dict(n=n, seed=n, clamp=True)))


def scene(name):
    """The scene `name` of SCENES, from its seed: dict(means3D, colors, opacities, scales, rotations, settings)."""
    from gsvc_amd import synthetic
    kind, kw = SCENES[name]()
    if kind == "stacked":
        return _stacked(**kw)
    if kind == "big":
        return _big(**kw)
    sc = synthetic.raster_scene(kw["P"], H=kw["H"], W=kw["W"], T=64, seed=kw["seed"], window_frames=8, sigma_px=kw["sigma_px"])
    return _needles(sc) if kind == "needles" else sc


def borderline_cap(name):
    return 5e-3 if name.startswith("S") else 5e-4


def oracle_settings(oracle, s, view="viewmatrix", bg=None, flags=None):
    return oracle.make_settings(s["H"], s["W"], s["x_min"], s["y_min"], s["scale"], s["threshold"], s[view],
                                bg=bg if bg is not None else s["bg"], scale_modifier=s["scale_modifier"],
                                flags=s.get("flags", 0) if flags is None else flags, low_pass=s.get("low_pass", 0.0))


def oracle_forward(oracle, sc, bg=(0.0, 0.0, 0.0), flags=None, view="viewmatrix"):
    s = sc["settings"]
    return oracle.raster_forward(oracle_settings(oracle, s, view, bg, flags), sc["means3D"], sc["colors"], sc["opacities"], sc["scales"],
                                 sc["rotations"])
