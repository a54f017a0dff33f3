"""NumPy restatement of the resampler's arithmetic (gsvc_amd/resample.py's docstring; include/gsvc_hip.h, gsvc_resample_frames).  It takes
the tables (``first``, ``coef``, ``nt`` of one axis) and restates the formulas on int64, plane by plane; and, for the accuracy checks,
the same filter in float64 with weights that were never quantised, built here from the formula and not from the product's code."""
import math

import numpy as np


def plane_dims(H, W, layout):
    ch, cw = (H // 2, W // 2) if layout == "yuv420p" else (H, W)
    return ((H, W), (ch, cw), (ch, cw))


def resample_plane(a, tx, ty, depth):
    """One plane ``a`` (integers ``[h, w]``) through the x table ``tx`` and the y table ``ty`` (each ``(first, coef, nt)``) -> int64
    ``[len(first_y), len(first_x)]``.  Slots at and beyond ``nt`` are not looked at."""
    a = np.asarray(a).astype(np.int64)
    h, w = a.shape
    d = int(depth)
    fx, cx, ntx = tx
    fy, cy, nty = ty
    cx = np.asarray(cx)[:, :ntx].astype(np.int64)
    cy = np.asarray(cy)[:, :nty].astype(np.int64)
    ix = np.clip(np.asarray(fx).astype(np.int64)[:, None] + np.arange(ntx), 0, w - 1)          # [ow, ntx]
    t = (a[:, ix] * cx[None]).sum(axis=2)                                                        # [h, ow]
    m = (t + (1 << (d - 3))) >> (d - 2)
    iy = np.clip(np.asarray(fy).astype(np.int64)[:, None] + np.arange(nty), 0, h - 1)          # [oh, nty]
    u = (m[iy] * cy[:, :, None]).sum(axis=1)                                                     # [oh, ow]
    return np.clip((u + (1 << (29 - d))) >> (30 - d), 0, (1 << d) - 1)


def resample_frame(buf, H, W, layout, depth, out_H, out_W, taps):
    """One flat frame (uint8 array of the frame's bytes) -> the flat uint8 frame at ``out_H x out_W``.  ``taps(src, dst)`` returns the
    table of one axis."""
    buf = np.ascontiguousarray(buf, np.uint8)
    codes = buf.view("<u2") if depth > 8 else buf
    out, at = [], 0
    for (h, w), (oh, ow) in zip(plane_dims(H, W, layout), plane_dims(out_H, out_W, layout)):
        plane = codes[at:at + h * w].reshape(h, w)
        at += h * w
        out.append(resample_plane(plane, taps(w, ow), taps(h, oh), depth).reshape(-1))
    flat = np.concatenate(out)
    return flat.astype("<u2").view(np.uint8) if depth > 8 else flat.astype(np.uint8)


def resample_frames(frames, H, W, layout, depth, out_H, out_W, taps):
    return np.stack([resample_frame(f, H, W, layout, depth, out_H, out_W, taps) for f in frames])


# ---- the float64 filter with unquantised weights ----------------------------------------------------------------------------------
def _lanczos3(x):
    if x == 0.0:
        return 1.0
    if abs(x) >= 3.0:
        return 0.0
    return 3.0 * math.sin(math.pi * x) * math.sin(math.pi * x / 3.0) / (math.pi * math.pi * x * x)


def float_matrix(src, dst):
    """The ``[dst, src]`` float64 matrix of one axis: normalised Lanczos-3 weights, taps outside the plane added to its edge sample."""
    A = np.zeros((dst, src), np.float64)
    M = max(src, dst)
    for j in range(dst):
        P = (2 * j + 1) * src - dst
        lo = (P - 6 * M) // (2 * dst) + 1
        hi = -((-(P + 6 * M)) // (2 * dst)) - 1
        w = np.array([_lanczos3((2 * dst * i - P) / (2.0 * M)) for i in range(lo, hi + 1)])
        w /= w.sum()
        for i, v in zip(range(lo, hi + 1), w):
            A[j, min(max(i, 0), src - 1)] += v
    return A


def float_resample_plane(a, out_h, out_w, depth):
    """The plane filtered in float64, clipped to the code range at the end only, not rounded."""
    a = np.asarray(a, np.float64)
    h, w = a.shape
    return np.clip(float_matrix(h, out_h) @ a @ float_matrix(w, out_w).T, 0.0, float((1 << depth) - 1))
