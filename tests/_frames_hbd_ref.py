"""float64 reference of the frame stages at any sample depth d (numpy), both directions, written from the formulas of
include/gsvc_hip.h (gsvc_frames_to_u8 / _to_u16 / _from_u8 / _from_u16), not from the kernels and not from the two 8-bit references
(tests/_frames_ref.py, tests/_frames_in_ref.py), which it must reproduce exactly at d = 8 (tests/test_frames_hbd_cpu.py).

Codes are numbers here, not bytes: a frame is a flat array of H W 3 (yuv444p) or H W 3 / 2 (yuv420p) codes in plane order Y, U, V; the
tests turn it into the little-endian 16-bit words (or, at d = 8, the bytes) of a frame buffer with ``to_bytes`` / ``from_bytes``.

Tolerances of tests/test_frames_hbd_gpu.py, the 8-bit tests' rules scaled with the code range (``check_codes``): a code b against the
float64 value v before rounding — nearest |b - v| <= 0.5 + delta, trunc v - 1 - delta < b <= v + delta, delta = 2^(d - 19) (2^-11 at
d = 8: float32 carries a value below 2^d to 2^(d - 24), and the matrix and the affine map are a handful of such roundings).  Input:
2^-20 absolute on every float, the 8-bit bound (the quotients do not depend on d beyond their own rounding)."""
import numpy as np

MATRIX = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}
TOL_IN = 2.0 ** -20


def constants(depth, rng):
    """(y_off, y_scale, c_off, c_scale, top) of the affine map code = off + scale * value."""
    up, top = float(2 ** (depth - 8)), float(2 ** depth - 1)
    if rng == "limited":
        return 16.0 * up, 219.0 * up, float(2 ** (depth - 1)), 224.0 * up, top
    assert rng == "full"
    return 0.0, top, float(2 ** (depth - 1)), top, top


def frame_codes(H, W, layout):
    return H * W * 3 // 2 if layout == "yuv420p" else 3 * H * W


def to_bytes(codes, depth):
    """Flat codes -> the uint8 buffer of a frame: bytes at d = 8, little-endian 16-bit words above."""
    c = np.asarray(codes)
    return c.astype(np.uint8) if depth == 8 else c.astype("<u2").view(np.uint8)


def from_bytes(buf, depth):
    b = np.ascontiguousarray(np.asarray(buf, dtype=np.uint8)).reshape(-1)
    return b.astype(np.int64) if depth == 8 else b.view("<u2").astype(np.int64)


# ---- output: images -> codes -------------------------------------------------------------------------------------------------------
def values(img, layout, matrix="bt709", rng="limited", depth=8):
    """img [3, H, W] (NaN / inf allowed) -> flat float64 samples BEFORE rounding, clamped to [0, 2^d - 1], in plane order."""
    x = np.asarray(img, dtype=np.float64)
    c = np.where(x > 0, x, 0.0)          # NaN, -inf -> 0
    c = np.minimum(c, 1.0)               # +inf -> 1
    _, H, W = c.shape
    Kr, Kb = MATRIX[matrix]
    Kg = 1.0 - Kr - Kb
    R, G, B = c
    Y = Kr * R + Kg * G + Kb * B
    Cb = (B - Y) / (2.0 * (1.0 - Kb))
    Cr = (R - Y) / (2.0 * (1.0 - Kr))
    if layout == "yuv420p":
        assert H % 2 == 0 and W % 2 == 0
        Cb = Cb.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))
        Cr = Cr.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))
    else:
        assert layout == "yuv444p"
    y_off, y_scale, c_off, c_scale, top = constants(depth, rng)
    v = np.concatenate([(y_off + y_scale * Y).reshape(-1), (c_off + c_scale * Cb).reshape(-1), (c_off + c_scale * Cr).reshape(-1)])
    return np.clip(v, 0.0, top)


def quantise(v, rounding):
    if rounding == "trunc":
        return np.floor(v).astype(np.int64)
    assert rounding == "nearest"
    return np.floor(v + 0.5).astype(np.int64)


def convert(img, layout, matrix="bt709", rng="limited", rounding="nearest", depth=8):
    return quantise(values(img, layout, matrix, rng, depth), rounding)


def check_codes(got, v, rounding, depth):
    """Number of codes that break the condition of the module's text, and the worst excess."""
    delta = 2.0 ** (depth - 19)
    b = np.asarray(got, dtype=np.float64).reshape(-1)
    assert b.shape == v.shape, (b.shape, v.shape)
    if rounding == "nearest":
        excess = np.abs(b - v) - (0.5 + delta)
        bad = excess > 0
    else:
        bad = ~((v - 1.0 - delta < b) & (b <= v + delta))
        excess = np.maximum(b - v - delta, v - 1.0 - delta - b)
    return int(bad.sum()), float(excess.max()) if excess.size else 0.0


# ---- input: codes -> images --------------------------------------------------------------------------------------------------------
def split(codes, H, W, layout):
    flat = np.asarray(codes).reshape(-1)
    assert flat.shape[0] == frame_codes(H, W, layout), (flat.shape, H, W, layout)
    ch, cw = (H // 2, W // 2) if layout == "yuv420p" else (H, W)
    return flat[:H * W].reshape(H, W), flat[H * W:H * W + ch * cw].reshape(ch, cw), flat[H * W + ch * cw:].reshape(ch, cw)


def upsample_codes(c, chroma):
    """[H / 2, W / 2] codes -> float64 [H, W]; centre sited.  ``nearest``: each sample serves its 2x2 block.  ``bilinear``, per axis:
    position 2 j takes 0.25 c[j - 1] + 0.75 c[j], position 2 j + 1 takes 0.75 c[j] + 0.25 c[j + 1], indices clamped."""
    c = np.asarray(c, dtype=np.float64)
    h, w = c.shape
    if chroma == "nearest":
        return c[np.arange(2 * h) // 2][:, np.arange(2 * w) // 2]
    assert chroma == "bilinear"

    def taps(n):
        p = np.arange(2 * n)
        near = p // 2
        far = np.clip(np.where(p % 2 == 1, near + 1, near - 1), 0, n - 1)
        return near, far

    ni, fi = taps(h)
    nj, fj = taps(w)
    rows = 0.75 * c[ni] + 0.25 * c[fi]
    return 0.75 * rows[:, nj] + 0.25 * rows[:, fj]


def rgb_of_codes(y, cb, cr, matrix="bt709", rng="limited", depth=8):
    """Codes (arrays of one shape; chroma codes may be interpolated) -> float64 [3, ...] R, G, B clamped to [0, 1]."""
    Kr, Kb = MATRIX[matrix]
    Kg = 1.0 - Kr - Kb
    y_off, y_scale, c_off, c_scale, _ = constants(depth, rng)
    y, cb, cr = (np.asarray(v, dtype=np.float64) for v in (y, cb, cr))
    Y, Cb, Cr = (y - y_off) / y_scale, (cb - c_off) / c_scale, (cr - c_off) / c_scale
    R = Y + 2.0 * (1.0 - Kr) * Cr
    B = Y + 2.0 * (1.0 - Kb) * Cb
    G = Y - (2.0 * Kr * (1.0 - Kr) / Kg) * Cr - (2.0 * Kb * (1.0 - Kb) / Kg) * Cb
    return np.clip(np.stack([R, G, B]), 0.0, 1.0)


def image(codes, H, W, layout, matrix="bt709", rng="limited", chroma="bilinear", depth=8):
    """One frame's flat codes -> float64 [3, H, W]."""
    y, u, v = split(codes, H, W, layout)
    if layout == "yuv420p":
        u, v = upsample_codes(u, chroma), upsample_codes(v, chroma)
    return rgb_of_codes(y, u, v, matrix, rng, depth)


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------
def make_images(n, H, W, depth, seed=0):
    """float32 [n, 3, H, W]: uniform in [-0.1, 1.1], with the exact values 0, 1 and k / (2^d - 1) sprinkled over a quarter of the elements."""
    rng = np.random.default_rng(9000 + seed)
    img = rng.uniform(-0.1, 1.1, (n, 3, H, W)).astype(np.float32)
    pick = rng.random(img.shape) < 0.25
    top = 2 ** depth - 1
    k = rng.integers(0, top + 1, img.shape)
    k[rng.random(img.shape) < 0.2] = 0
    k[rng.random(img.shape) < 0.2] = top
    exact = (k.astype(np.float32) / np.float32(top)).astype(np.float32)
    img[pick] = exact[pick]
    return img


def random_codes(H, W, layout, depth, seed):
    return np.random.default_rng(9500 + seed).integers(0, 2 ** depth, frame_codes(H, W, layout), dtype=np.int64)
