"""NumPy statement of the frame histograms (include/gsvc_hip.h, gsvc_frames_histogram) and of the histogram distance of
gsvc_amd/scene.py: for plane p of a frame, ``hist[p, b]`` = the number of samples whose code c has ``min(c >> (depth - 8), 255) == b``
(``np.bincount`` per plane), and ``d[t] = sum_b |h[t + 1, b] - h[t, b]| / (2 samples)`` on the luma plane folded to ``bins`` bins, as
Python integers before the one division."""
import numpy as np

from tests._picture_hash_ref import frame_planes


def histogram_ref(frames_u8, H, W, layout, depth):
    """uint8 [n, >= frame_bytes] -> int64 [n, 3, 256]."""
    frames_u8 = np.asarray(frames_u8)
    out = np.zeros((frames_u8.shape[0], 3, 256), np.int64)
    for k in range(frames_u8.shape[0]):
        for p, codes in enumerate(frame_planes(frames_u8[k], H, W, layout, depth)):
            bins = np.minimum(codes.astype(np.int64) >> (depth - 8), 255)
            out[k, p] = np.bincount(bins, minlength=256)
    return out


def distance_ref(hist, bins=64, layout="yuv420p"):
    """[n, 3, 256] -> a list of n - 1 floats, each ONE division of two Python integers."""
    luma = np.asarray(hist)[:, 1 if layout == "rgb24" else 0].astype(np.int64)
    group = 256 // bins
    out = []
    for t in range(luma.shape[0] - 1):
        a = [int(luma[t, g * group:(g + 1) * group].sum()) for g in range(bins)]
        b = [int(luma[t + 1, g * group:(g + 1) * group].sum()) for g in range(bins)]
        out.append(sum(abs(x - y) for x, y in zip(a, b)) / (2 * sum(a)))
    return out
