"""Numpy restatement of gsvc_amd/grain.py, written from its docstring: the synthesis (``white``, ``filtered``, ``apply_ref``), the
flat-block statistics (``stats_ref``) and the fit (``fit_ref``).  Nothing here imports the library or needs a GPU."""
import math

import numpy as np

GOLD = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
    return z ^ (z >> np.uint64(31))


def white(seed: int, f: int, p: int, y0: int, y1: int, x0: int, x1: int) -> np.ndarray:
    """g(y, x) for y0 <= y < y1, x0 <= x < x1 (both from -1) as int64 ``[y1 - y0, x1 - x0]``."""
    with np.errstate(over="ignore"):
        key = mix(np.array([seed], np.uint64) + np.array([3 * f + p + 1], np.uint64) * GOLD)[0]
        Y = (np.arange(y0, y1, dtype=np.int64) + 1).astype(np.uint64)[:, None]
        X = (np.arange(x0, x1, dtype=np.int64) + 1).astype(np.uint64)[None, :]
        h = mix(key + ((Y << np.uint64(32)) | (X >> np.uint64(1))) * GOLD)
    w = np.where((X & np.uint64(1)) == 1, h >> np.uint64(32), h & np.uint64(0xFFFFFFFF))
    total = sum((w >> np.uint64(8 * k)) & np.uint64(255) for k in range(4))
    return total.astype(np.int64) - 510


def filtered(seed: int, f: int, p: int, h: int, w: int, kx: int, ky: int) -> np.ndarray:
    """n(y, x) of an h x w plane, int64."""
    g = white(seed, f, p, -1, h + 1, -1, w + 1)
    t = kx * (g[:, :-2] + g[:, 2:]) + 64 * g[:, 1:-1]
    return (ky * (t[:-2] + t[2:]) + 64 * t[1:-1] + 2048) >> 12


def plane_views(frame: np.ndarray, H: int, W: int, layout: str, depth: int):
    """Views (y, u, v) into one flat uint8 frame; deep frames as '<u2'."""
    ch, cw = (H // 2, W // 2) if layout == "yuv420p" else (H, W)
    n = (H * W + 2 * ch * cw) * (2 if depth > 8 else 1)
    flat = frame[:n]
    if depth > 8:
        flat = flat.view("<u2")
    return flat[:H * W].reshape(H, W), flat[H * W:H * W + ch * cw].reshape(ch, cw), flat[H * W + ch * cw:].reshape(ch, cw)


def nominal(p: int, depth: int, rng: str):
    up = 1 << (depth - 8)
    return (16 * up, (235 if p == 0 else 240) * up) if rng == "limited" else (0, (1 << depth) - 1)


def apply_ref(frames: np.ndarray, H: int, W: int, layout: str, depth: int, rng: str, seed: int, scale, kx, ky, frame_ids) -> np.ndarray:
    """uint8 ``[n, >= frame_bytes]`` -> a grained copy (bytes beyond the frame are copied as they are)."""
    out = frames.copy()
    S = 24 - depth
    for k, f in enumerate(frame_ids):
        src, dst = plane_views(frames[k], H, W, layout, depth), plane_views(out[k], H, W, layout, depth)
        luma = src[0].astype(np.int64)
        for p in range(3):
            c = src[p].astype(np.int64)
            if p == 0 or layout == "yuv444p":
                m = luma
            else:
                m = (luma[0::2, 0::2] + luma[0::2, 1::2] + luma[1::2, 0::2] + luma[1::2, 1::2] + 2) >> 2
            l = np.minimum(m >> (depth - 8), 255)
            i, r = l >> 4, l & 15
            sc = np.asarray(scale[p], np.int64)
            s = (sc[i] * (16 - r) + sc[i + 1] * r + 8) >> 4
            n = filtered(seed, int(f), p, c.shape[0], c.shape[1], int(kx[p]), int(ky[p]))
            grain = (n * s + (1 << (S - 1))) >> S
            lo, hi = nominal(p, depth, rng)
            dst[p][...] = np.minimum(np.maximum(c + grain, np.minimum(lo, c)), np.maximum(hi, c)).astype(dst[p].dtype)
    return out


def stats_ref(src: np.ndarray, dec: np.ndarray, H: int, W: int, layout: str, depth: int, flat_threshold: int, max_residual: int) -> np.ndarray:
    """int64 ``[3, 16, 6]`` over the frames of two uint8 ``[n, >= frame_bytes]`` buffers."""
    out = np.zeros((3, 16, 6), np.int64)
    up = 1 << (depth - 8)
    for k in range(src.shape[0]):
        ps, pd = plane_views(src[k], H, W, layout, depth), plane_views(dec[k], H, W, layout, depth)
        dluma = pd[0].astype(np.int64)
        for p in range(3):
            s, d = ps[p].astype(np.int64), pd[p].astype(np.int64)
            sub = p > 0 and layout == "yuv420p"
            for by in range(d.shape[0] // 8):
                for bx in range(d.shape[1] // 8):
                    db = d[8 * by:8 * by + 8, 8 * bx:8 * bx + 8]
                    r = s[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] - db
                    A = int(np.abs(db[:, 1:] - db[:, :-1]).sum() + np.abs(db[1:] - db[:-1]).sum())
                    if sub:
                        lum = int(dluma[16 * by:16 * by + 16, 16 * bx:16 * bx + 16].sum()) >> 8
                    elif p == 0:
                        lum = int(db.sum()) >> 6
                    else:
                        lum = int(dluma[8 * by:8 * by + 8, 8 * bx:8 * bx + 8].sum()) >> 6
                    b = min(lum >> (depth - 8), 255) >> 4
                    if A > flat_threshold * up or int(np.abs(r).max()) > max_residual * up:
                        continue
                    S1 = int(r.sum())
                    out[p, b] += np.array([1, S1, int((r * r).sum()), S1 * S1, int((r[:, :-1] * r[:, 1:]).sum()), int((r[:-1] * r[1:]).sum())],
                                          np.int64)
    return out


# ---- the fit -------------------------------------------------------------------------------------------------------------------
def noise_variance(kx, ky):
    return 21845.0 * (4096 + 2 * kx * kx) * (4096 + 2 * ky * ky) / 2.0 ** 24


def lag1(k):
    return 128.0 * k / (4096.0 + 2.0 * k * k)


def lag2(k):
    return 1.0 * k * k / (4096.0 + 2.0 * k * k)


def dc_share(kx, ky):
    mx = 1.0 + (14.0 * lag1(kx) + 12.0 * lag2(kx)) / 8.0
    my = 1.0 + (14.0 * lag1(ky) + 12.0 * lag2(ky)) / 8.0
    return mx * my / 64.0


def fit_ref(stats, gain: float = 1.0, min_blocks: int = 16, depth: int = 8):
    """-> (scale [3][17], kx [3], ky [3]) as lists of ints, as ``fit_grain``'s docstring describes them."""
    rows = np.asarray(stats, dtype=object)
    up = float(1 << (depth - 8))
    taps = np.arange(-32, 33)
    KX, KY = np.meshgrid(taps, taps, indexing="ij")
    E = dc_share(KX.astype(np.float64), KY.astype(np.float64))
    PX, PY = (lag1(KX.astype(np.float64)) - E) / (1 - E), (lag1(KY.astype(np.float64)) - E) / (1 - E)
    scale, kxs, kys = [], [], []
    for p in range(3):
        ok = [b for b in range(16) if int(rows[p][b][0]) >= max(min_blocks, 1)]
        if not ok:
            scale.append([0] * 17)
            kxs.append(0)
            kys.append(0)
            continue
        N, S2, Q, Px, Py = (sum(int(rows[p][b][j]) for b in ok) for j in (0, 2, 3, 4, 5))
        V = (S2 - Q / 64.0) / (64.0 * N)
        kx = ky = 0
        if V > 0:
            rx, ry = (Px - 56.0 * Q / 4096.0) / (56.0 * N) / V, (Py - 56.0 * Q / 4096.0) / (56.0 * N) / V
            D = (PX - rx) ** 2 + (PY - ry) ** 2
            ix, iy = np.unravel_index(int(np.argmin(D)), D.shape)          # (row-major: the first minimum in kx, then ky, order)
            kx, ky = int(taps[ix]), int(taps[iy])
        e = dc_share(kx, ky)
        unit = math.sqrt(noise_variance(kx, ky))
        val = {}
        for b in ok:
            n_b, s2, q = int(rows[p][b][0]), int(rows[p][b][2]), int(rows[p][b][3])
            var = max((s2 - q / 64.0) / (64.0 * n_b) / (1.0 - e) - 1.0 / 12.0, 0.0)
            val[b] = gain * math.sqrt(var) / up * 65536.0 / unit
        full = list(np.interp(np.arange(16), ok, [val[b] for b in ok]))      # (linear between, the end values beyond)
        knots = [full[0]] + [(full[i - 1] + full[i]) / 2.0 for i in range(1, 16)] + [full[15]]
        scale.append([min(int(round(v)), 65535) for v in knots])
        kxs.append(kx)
        kys.append(ky)
    return scale, kxs, kys


def flat_sigma(stats):
    """Per plane and bin the block-DC-removed standard deviation sqrt((S2 - S1^2 / 64) / (64 N)), NaN without blocks."""
    rows = np.asarray(stats, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(np.maximum((rows[..., 2] - rows[..., 3] / 64.0) / (64.0 * rows[..., 0]), 0.0))


# ---- the closed loop both test files run: flat patches + grain -> statistics -> fit ------------------------------------------------
def closed_loop_case():
    """Four 256 x 256 full-range yuv420p frames of flat patches — 16 luma bands of 16 rows at the bin centres 8, 24, .., 248, chroma at 128 —
    and the parameters whose grain is put on them: {"H", "W", "layout", "depth", "range", "dec" (uint8 [4, frame_bytes]), "seed", "scale",
    "kx", "ky", "frame_ids"}.  Luma: 256 blocks per bin; chroma: 64."""
    H = W = 256
    T = 4
    luma = np.repeat(np.arange(16, dtype=np.uint8) * 16 + 8, 16)[:, None].repeat(W, axis=1)
    frame = np.concatenate([luma.reshape(-1), np.full(2 * (H // 2) * (W // 2), 128, np.uint8)])
    scale = [[600 + 40 * i for i in range(17)], [900] * 17, [1400 - 30 * i for i in range(17)]]
    return {"H": H, "W": W, "layout": "yuv420p", "depth": 8, "range": "full", "dec": np.tile(frame, (T, 1)), "seed": 0x5EEDF00DCAFE,
            "scale": scale, "kx": [16, 0, -12], "ky": [8, 0, 20], "frame_ids": [7, 8, 9, 10]}


def interp_scale(row, l):
    return (row[l >> 4] * (16 - (l & 15)) + row[(l >> 4) + 1] * (l & 15) + 8) >> 4


def recovery_error(case, scale, kx, ky):
    """(the largest relative error of a recovered strength, the largest error of a recovered tap).  Interior knots are compared with the
    knots put in, the two end knots with the input's strength at the centre of the first / last bin (what the fit defines them as)."""
    rel = 0.0
    for p in range(3):
        want = [interp_scale(case["scale"][p], 8)] + list(case["scale"][p][1:16]) + [interp_scale(case["scale"][p], 248)]
        rel = max(rel, max(abs(g - w) / w for g, w in zip(scale[p], want)))
    tap = max(max(abs(a - b) for a, b in zip(kx, case["kx"])), max(abs(a - b) for a, b in zip(ky, case["ky"])))
    return rel, tap


# measured with this file on the CPU (tests/test_grain_cpu.py prints them): the recovery error of the reference itself on closed_loop_case()
CLOSED_LOOP_MEASURED = (0.02567, 0)          # strengths within 2.567 %, every tap exact
CLOSED_LOOP_BOUND = (2 * CLOSED_LOOP_MEASURED[0], 2 * CLOSED_LOOP_MEASURED[1])
