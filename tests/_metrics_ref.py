"""Float64 / exact-integer NumPy statements of the video metrics of gsvc_amd.metrics (csrc/metrics.hip; formulas: include/gsvc_hip.h),
the seeded pictures the MS-SSIM tests run on, and the two bounds those tests hold the kernel to.

MS-SSIM: 11-tap Gaussian window (sigma 1.5) applied separably without padding, 5 scales, 2x2 mean between scales with ONE leading
zero row / column on an odd side (divisor 4), K = (0.01, 0.03), data range 1.  ``ms_ssim_ref`` returns the five per-plane means
(contrast-structure at scales 0 .. 3, SSIM at scale 4, unclipped) and the final value per plane.
"""
import functools

import numpy as np

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2


# ---- MS-SSIM in float64 ----------------------------------------------------------------------------------------------------
def window():
    x = np.arange(11, dtype=np.float64) - 5
    g = np.exp(-(x ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def blur_valid(a, g=None):
    """Valid separable convolution over the last two axes: [..., h, w] -> [..., h - 10, w - 10]."""
    g = window() if g is None else g
    k = g.shape[0]
    h, w = a.shape[-2:]
    v = sum(g[i] * a[..., i:h - k + 1 + i, :] for i in range(k))
    return sum(g[i] * v[..., :, i:w - k + 1 + i] for i in range(k))


def pool2(a):
    """2x2 mean over the last two axes; an odd side gets one leading zero row / column (its first window covers -1 and 0)."""
    h, w = a.shape[-2:]
    p = np.zeros(a.shape[:-2] + (h + h % 2, w + w % 2), a.dtype)
    p[..., h % 2:, w % 2:] = a
    return (p[..., 0::2, 0::2] + p[..., 0::2, 1::2] + p[..., 1::2, 0::2] + p[..., 1::2, 1::2]) / 4


def pyramid(a):
    """The five scales of [..., H, W]."""
    out = [np.asarray(a, np.float64)]
    for _ in range(4):
        out.append(pool2(out[-1]))
    return out


def ssim_cs_maps(x, y):
    mu1, mu2 = blur_valid(x), blur_valid(y)
    s1 = blur_valid(x * x) - mu1 * mu1
    s2 = blur_valid(y * y) - mu2 * mu2
    s12 = blur_valid(x * y) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    return ((2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1)) * cs, cs


def ms_ssim_ref(x, y):
    """x, y [..., H, W] -> (terms float64 [5, ...], value float64 [...]); value = prod relu(terms) ** weights."""
    px, py = pyramid(x), pyramid(y)
    terms = []
    for k in range(5):
        ssim, cs = ssim_cs_maps(px[k], py[k])
        terms.append((ssim if k == 4 else cs).mean(axis=(-2, -1)))
    terms = np.stack(terms)
    w = np.asarray(MS_WEIGHTS).reshape((5,) + (1,) * (terms.ndim - 1))
    return terms, np.prod(np.maximum(terms, 0.0) ** w, axis=0)


def torch_terms(x, y, dtype):
    """The arithmetic of ``gsvc_amd.metrics.ms_ssim`` (its own helpers, its loop restated so that the five means come out) on tensors
    cast to ``dtype``: (terms [5, N, C], value [N, C]).  float32 on the CPU = what the bounds below are measured on."""
    import torch
    import torch.nn.functional as F

    from gsvc_amd import metrics as M
    x, y = x.to(dtype), y.to(dtype)
    win = M._gauss_window(11, 1.5, x.device, dtype)
    terms = []
    for i in range(5):
        ssim_c, cs = M._ssim_cs(x, y, win, 1.0)
        terms.append(ssim_c if i == 4 else cs)
        if i < 4:
            pad = [s % 2 for s in x.shape[2:]]
            x, y = F.avg_pool2d(x, kernel_size=2, padding=pad), F.avg_pool2d(y, kernel_size=2, padding=pad)
    terms = torch.stack(terms)
    w = torch.tensor(MS_WEIGHTS, dtype=dtype).view(-1, 1, 1)
    return terms, torch.prod(torch.relu(terms) ** w, dim=0)


# ---- the pictures of the MS-SSIM tests ------------------------------------------------------------------------------------------
SHAPES = ((1, 1, 161, 163),          # every scale odd in both directions, 11 x 11 at the end
          (1, 1, 176, 161),
          (1, 1, 162, 330),          # more than one tile across, an even / odd mix
          (2, 3, 200, 181))          # a batch of images with three channels
FAMILIES = ("smooth", "uniform", "flat")
SIGMAS = (0.002, 0.02, 0.1)
CASES = tuple((s, f, g) for s in range(len(SHAPES)) for f in FAMILIES for g in SIGMAS)


def _quant8(a):
    return np.rint(np.clip(a, 0.0, 1.0) * 255.0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def picture_codes(shape_id, family, sigma):
    """(x, y) uint8 [N, C, H, W]: a smooth picture, uniform noise or a flat 0.7, and the same plus Gaussian noise of ``sigma``; both
    rounded to 8-bit codes.  Seeded by the case."""
    N, C, H, W = SHAPES[shape_id]
    rng = np.random.default_rng(1000 * shape_id + 100 * FAMILIES.index(family) + SIGMAS.index(sigma))
    if family == "smooth":
        i = np.arange(H, dtype=np.float64)[:, None] / H
        j = np.arange(W, dtype=np.float64)[None, :] / W
        ph = rng.uniform(0.0, 2 * np.pi, size=(N, C, 1, 1))
        base = 0.5 + 0.25 * np.sin(2 * np.pi * 1.5 * i + ph) * np.cos(2 * np.pi * j + ph) + 0.15 * (j - 0.5)
    elif family == "uniform":
        base = rng.uniform(0.0, 1.0, size=(N, C, H, W))
    else:
        base = np.full((N, C, H, W), 0.7)
    noisy = base + rng.normal(0.0, sigma, size=(N, C, H, W))
    x, y = _quant8(base), _quant8(noisy)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def reference(shape_id, family, sigma):
    """(terms [5, N, C], value [N, C]) of the float64 statement on ``picture_codes`` / 255; computed once per case, read-only."""
    x, y = picture_codes(shape_id, family, sigma)
    t, v = ms_ssim_ref(x.astype(np.float64) / 255.0, y.astype(np.float64) / 255.0)
    t.setflags(write=False)
    v.setflags(write=False)
    return t, v


def measure_float32_error():
    """(worst |term - float64|, worst |value - float64|) of the float32 tensor expressions (``torch_terms`` on the CPU) over CASES.
    How the two constants below were obtained: ``python -c "import tests._metrics_ref as r; print(r.measure_float32_error())"``."""
    import torch
    worst_t = worst_v = 0.0
    for case in CASES:
        x, y = picture_codes(*case)
        rt, rv = reference(*case)
        t, v = torch_terms(torch.from_numpy(x.astype(np.float32) / np.float32(255.0)), torch.from_numpy(y.astype(np.float32) / np.float32(255.0)),
                           torch.float32)
        worst_t = max(worst_t, float(np.abs(t.double().numpy() - rt).max()))
        worst_v = max(worst_v, float(np.abs(v.double().numpy() - rv).max()))
    return worst_t, worst_v


# The bounds of tests/test_metrics_gpu.py: 2 x the error of the float32 tensor expressions (metrics.ms_ssim's arithmetic, run on the
# CPU) against the float64 statement above, the worst over exactly CASES — measure_float32_error() gave
#     per-scale term  8.73e-5     final value  3.77e-5
# (both on the flat 0.7 with sigma 0.002 at 200 x 181: E[x^2] - mu^2 subtracts two numbers near 0.49 to get one near 4e-6; the smooth
# pictures stay below 9e-6 and 4e-6).  The constants are these figures rounded DOWN to two digits.
# The factor 2 covers another summation order, not another algorithm.
F32_TERM_ERROR = 8.7e-5
F32_VALUE_ERROR = 3.7e-5
TERM_BOUND = 2 * F32_TERM_ERROR
VALUE_BOUND = 2 * F32_VALUE_ERROR


# ---- SSE and PSNR on codes ------------------------------------------------------------------------------------------------------
def plane_slices(H, W, layout):
    px = H * W
    c = px // 4 if layout == "yuv420p" else px
    return (slice(0, px), slice(px, px + c), slice(px + c, px + 2 * c))


def sse_ref(a, b, H, W, layout, depth):
    """a, b uint8 [n, >= frame_bytes] -> int64 [n, 3]: the sum of squared code differences per plane (rgb24: per channel)."""
    per = 2 if depth > 8 else 1
    samples = (H * W * 3 // 2 if layout == "yuv420p" else 3 * H * W)
    out = np.zeros((a.shape[0], 3), np.int64)
    for k in range(a.shape[0]):
        ca = np.ascontiguousarray(a[k, :samples * per]).view("<u2" if per == 2 else np.uint8).astype(np.int64)
        cb = np.ascontiguousarray(b[k, :samples * per]).view("<u2" if per == 2 else np.uint8).astype(np.int64)
        d2 = (ca - cb) ** 2
        if layout == "rgb24":
            out[k] = d2.reshape(-1, 3).sum(0)
        else:
            out[k] = [d2[s].sum() for s in plane_slices(H, W, layout)]
    return out


def psnr_ref(sse, samples, peak):
    """10 log10(peak^2 samples / SSE) in float64; +inf where SSE is 0."""
    sse = np.asarray(sse, np.float64)
    with np.errstate(divide="ignore"):
        return np.where(sse > 0, 10.0 * np.log10(float(peak) ** 2 * np.asarray(samples, np.float64) / np.maximum(sse, 1e-300)), np.inf)
