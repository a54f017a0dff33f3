"""NumPy / Python-int statement of the detail map and of the point sampler (include/gsvc_hip.h, gsvc_frames_detail and
gsvc_detail_sample; gsvc_amd/detail.py).  The map is summed in int64; the sampler's hash in Python integers modulo 2^64.  The fmaf
forms are evaluated in float64 and rounded once to float32: exact here, because f cw + x0 (f a multiple of 2^-24 below 1, cw <= 16,
x0 < 2^15) fits in the 53 bits of a double."""
import numpy as np

M64 = (1 << 64) - 1
GOLD, MUL1, MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def luma_of(frames_u8, H, W, depth):
    """uint8 ``[n, >= frame bytes]`` -> int64 ``[n, H, W]``: the first H W samples of every frame, as they are."""
    a = np.ascontiguousarray(frames_u8)
    if depth > 8:
        return np.stack([row[:2 * H * W].view("<u2").astype(np.int64).reshape(H, W) for row in a])
    return a[:, :H * W].astype(np.int64).reshape(-1, H, W)


def detail_map_ref(luma, cell, n_out=None):
    """int64 luma ``[n, H, W]`` -> int64 ``[n_out, Hc, Wc]``."""
    Y = np.asarray(luma, np.int64)
    n, H, W = Y.shape
    n_out = n if n_out is None else n_out
    xs, ys = np.arange(W), np.arange(H)
    gx = np.abs(Y[:, :, np.minimum(xs + 1, W - 1)] - Y[:, :, np.maximum(xs - 1, 0)])
    gy = np.abs(Y[:, np.minimum(ys + 1, H - 1)] - Y[:, np.maximum(ys - 1, 0)])
    e = gx + gy
    for f in range(n):
        g = f + 1 if f + 1 < n else (f - 1 if n > 1 else None)
        if g is not None:
            e[f] += 2 * np.abs(Y[g] - Y[f])
    Hc, Wc = -(-H // cell), -(-W // cell)
    pad = np.zeros((n, Hc * cell, Wc * cell), np.int64)
    pad[:, :H, :W] = e
    return pad.reshape(n, Hc, cell, Wc, cell).sum(axis=(2, 4))[:n_out]


def hash_ref(seed, i, k):
    z = (seed + (5 * i + k + 1) * GOLD) & M64
    z = ((z ^ (z >> 30)) * MUL1) & M64
    z = ((z ^ (z >> 27)) * MUL2) & M64
    return z ^ (z >> 31)


def sample_ref(dmap, H, W, cell, N, seed, mix24):
    """int map ``[T, Hc, Wc]`` -> (float32 ``[N, 3]``, int32 ``[N]``)."""
    m = np.asarray(dmap, np.int64)
    T, Hc, Wc = m.shape
    cdf = np.cumsum(m.reshape(-1))
    D = int(cdf[-1])
    pts, at = np.empty((N, 3), np.float32), np.empty(N, np.int32)
    for i in range(N):
        h = [hash_ref(seed, i, k) for k in range(5)]
        if D == 0 or (h[0] >> 40) < mix24:
            p = (h[1] * (T * H * W)) >> 64
            t, q = divmod(p, H * W)
            y0, x0 = divmod(q, W)
            cw = ch = 1
            c = (t * Hc + y0 // cell) * Wc + x0 // cell
        else:
            r = (h[1] * D) >> 64
            c = int(np.searchsorted(cdf, r, side="right"))          # the first index with cdf[index] > r
            t, q = divmod(c, Hc * Wc)
            cy, cx = divmod(q, Wc)
            x0, y0 = cx * cell, cy * cell
            cw, ch = min(cell, W - x0), min(cell, H - y0)
        f2, f3, f4 = ((h[k] >> 40) * 2.0 ** -24 for k in (2, 3, 4))
        pts[i] = (np.float32(f2 * cw + x0), np.float32(f3 * ch + y0), np.float32((f4 - 0.5) + t))
        at[i] = c
    return pts, at


def quadrant_clip(seed=0):
    """The placement clip: 4 frames of 48 x 64 (H x W) yuv420p, luma 128 except random codes in rows 8 .. 15 and columns 8 .. 23 —
    detail strictly inside the top-left quadrant, one cell (8) from its border.  -> uint8 ``[4, 4608]``."""
    H, W, T = 48, 64, 4
    rng = np.random.default_rng(seed)
    frames = np.full((T, H * W * 3 // 2), 128, np.uint8)
    for t in range(T):
        y = frames[t, :H * W].reshape(H, W)
        y[8:16, 8:24] = rng.integers(0, 256, (8, 16), dtype=np.uint8)
    return frames
