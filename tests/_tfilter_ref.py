"""Numpy restatement of gsvc_amd/tfilter.py, written from its docstring in int64 and by the formulas (whole planes at a time, not a
wave per block): the vectors, the prediction, the block and sample weights, the output (``filter_planes``, ``filter_frames``), and the
noise sums (``noise_sums_ref``).  Nothing here imports the library or needs a GPU."""
import math

import numpy as np

OFFSETS = (-2, -1, 1, 2)


def luts():
    """The default tables, from the formulas."""
    b = [int(np.rint(256.0 * math.exp(-max(0, i - 16) / 8.0))) for i in range(64)]
    p = [int(np.rint(256.0 * math.exp(-((i / 8.0) ** 2) / 18.0))) for i in range(64)]
    return b, p


def vectors(flow) -> np.ndarray:
    """float32 ``[2, H, W]`` -> int64 ``[2, H, W]`` quarter pels: the float32 product rounded half to even, clamped to int16."""
    f = np.asarray(flow, dtype=np.float32)
    return np.clip(np.rint(np.float32(4.0) * f), -32768, 32767).astype(np.int64)


def predict(plane, mvx, mvy, unit: int) -> np.ndarray:
    """The prediction of every sample of ``plane`` (the neighbour's codes, int64 ``[h, w]``) from per-sample vectors in 1 / unit samples."""
    a = np.asarray(plane, dtype=np.int64)
    h, w = a.shape
    X, Y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    px, py = np.clip(unit * X + mvx, 0, unit * (w - 1)), np.clip(unit * Y + mvy, 0, unit * (h - 1))
    x0, y0 = np.minimum(px // unit, w - 2), np.minimum(py // unit, h - 2)
    fx, fy = px - unit * x0, py - unit * y0
    s = (unit - fx) * (unit - fy) * a[y0, x0] + fx * (unit - fy) * a[y0, x0 + 1] + (unit - fx) * fy * a[y0 + 1, x0] + fx * fy * a[y0 + 1, x0 + 1]
    return (s + unit * unit // 2) // (unit * unit)


def block_index(Y, pred, q0: int) -> np.ndarray:
    """i_b of every luma pixel ``[H, W]``: that of its 8 x 8 block (partial blocks count the pixels they have)."""
    H, W = Y.shape
    rows, cols = np.arange(0, H, 8), np.arange(0, W, 8)
    sse = np.add.reduceat(np.add.reduceat((Y - pred) ** 2, rows, axis=0), cols, axis=1)
    count = np.add.reduceat(np.add.reduceat(np.ones((H, W), np.int64), rows, axis=0), cols, axis=1)
    ib = np.minimum(63, 2048 * sse // (count * int(q0) ** 2))
    return np.repeat(np.repeat(ib, 8, axis=0), 8, axis=1)[:H, :W]


def filter_planes(clip, t: int, flows, q, wt, lut_b, lut_p, layout: str):
    """``clip``: a list of (Y, U, V) int64 planes; ``flows``: {d: float32 [2, H, W]} for every d of OFFSETS whose neighbour exists (others
    are not looked at).  Returns the filtered (Y, U, V) of frame t."""
    lut_b, lut_p = np.asarray(lut_b, np.int64), np.asarray(lut_p, np.int64)
    cur = [np.asarray(p, np.int64) for p in clip[t]]
    num = [256 * c for c in cur]
    den = [np.full(c.shape, 256, np.int64) for c in cur]
    sub = layout == "yuv420p"
    for d in OFFSETS:
        if not 0 <= t + d < len(clip):
            continue
        mv = vectors(flows[d])
        nb = [np.asarray(p, np.int64) for p in clip[t + d]]
        pred_y = predict(nb[0], mv[0], mv[1], 4)
        ib = block_index(cur[0], pred_y, q[0])
        for p in range(3):
            if p == 0:
                pred, ibp = pred_y, ib
            elif sub:
                pred, ibp = predict(nb[p], mv[0][0::2, 0::2], mv[1][0::2, 0::2], 8), ib[0::2, 0::2]
            else:
                pred, ibp = predict(nb[p], mv[0], mv[1], 4), ib
            ip = np.minimum(63, 128 * np.abs(cur[p] - pred) // int(q[p]))
            w = (int(wt[abs(d) - 1]) * lut_b[ibp] * lut_p[ip] + (1 << 15)) >> 16
            num[p] = num[p] + w * pred
            den[p] = den[p] + w
    return tuple((n + dn // 2) // dn for n, dn in zip(num, den))


def plane_views(frame: np.ndarray, H: int, W: int, layout: str, depth: int):
    """Views (y, u, v) into one flat uint8 frame; deep frames as '<u2'."""
    ch, cw = (H // 2, W // 2) if layout == "yuv420p" else (H, W)
    n = (H * W + 2 * ch * cw) * (2 if depth > 8 else 1)
    flat = frame[:n]
    if depth > 8:
        flat = flat.view("<u2")
    return flat[:H * W].reshape(H, W), flat[H * W:H * W + ch * cw].reshape(ch, cw), flat[H * W + ch * cw:].reshape(ch, cw)


def frame_bytes(H: int, W: int, layout: str, depth: int) -> int:
    ch, cw = (H // 2, W // 2) if layout == "yuv420p" else (H, W)
    return (H * W + 2 * ch * cw) * (2 if depth > 8 else 1)


def filter_frames(frames: np.ndarray, H: int, W: int, layout: str, depth: int, flows: np.ndarray, q, wt, lut_b, lut_p, first: int = 0):
    """uint8 ``[T, >= frame_bytes]`` and float32 ``[n, 4, 2, H, W]`` (slot j: OFFSETS[j]) -> uint8 ``[n, frame_bytes]``: the filtered frames
    first .. first + n - 1."""
    T, nb = frames.shape[0], frame_bytes(H, W, layout, depth)
    clip = [tuple(p.astype(np.int64) for p in plane_views(frames[t], H, W, layout, depth)) for t in range(T)]
    out = np.zeros((flows.shape[0], nb), np.uint8)
    for k in range(flows.shape[0]):
        got = filter_planes(clip, first + k, {d: flows[k, j] for j, d in enumerate(OFFSETS)}, q, wt, lut_b, lut_p, layout)
        for dst, plane in zip(plane_views(out[k], H, W, layout, depth), got):
            dst[...] = plane
    return out


def noise_sum(plane) -> int:
    c = np.asarray(plane, np.int64)
    lap = (c[:-2, :-2] - 2 * c[:-2, 1:-1] + c[:-2, 2:] - 2 * c[1:-1, :-2] + 4 * c[1:-1, 1:-1] - 2 * c[1:-1, 2:]
           + c[2:, :-2] - 2 * c[2:, 1:-1] + c[2:, 2:])
    return int(np.abs(lap).sum())


def noise_sums_ref(frames: np.ndarray, H: int, W: int, layout: str, depth: int) -> np.ndarray:
    """uint8 ``[n, >= frame_bytes]`` -> int64 ``[n, 3]``."""
    return np.array([[noise_sum(p) for p in plane_views(f, H, W, layout, depth)] for f in frames], np.int64)


def as_bytes(codes: np.ndarray, depth: int) -> np.ndarray:
    """int ``[n, samples]`` -> uint8 ``[n, bytes]``."""
    return np.ascontiguousarray(codes.astype("<u2" if depth > 8 else np.uint8)).view(np.uint8).reshape(codes.shape[0], -1)


def as_codes(frames: np.ndarray, depth: int) -> np.ndarray:
    """uint8 ``[n, bytes]`` -> the sample codes ``[n, samples]``."""
    a = np.ascontiguousarray(frames)
    return a.view("<u2") if depth > 8 else a


# ---- the test picture of the properties: a smooth pattern with one bright rectangle, 8-bit luma -------------------------------------
def pattern(H: int, W: int, shift: float = 0.0) -> np.ndarray:
    """float64 ``[H, W]`` clean codes, the content moved ``shift`` pixels to the right."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    x = x - shift
    img = 110.0 + 40.0 * np.sin(x / 11.0) * np.cos(y / 9.0) + 20.0 * np.sin((x + y) / 17.0)
    img = np.where((x >= 30) & (x < 55) & (y >= 20) & (y < 45), 215.0, img)
    return img


def clip_444(lumas) -> np.ndarray:
    """Luma planes -> uint8 ``[T, 3 H W]`` yuv444p 8-bit frames whose chroma planes repeat the luma."""
    return np.stack([np.concatenate([np.asarray(p, np.uint8).reshape(-1)] * 3) for p in lumas])
