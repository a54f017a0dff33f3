"""float64 reference of the encoder's 8-bit input stage (numpy), written from the formulas of include/gsvc_hip.h
(gsvc_frames_from_u8), not from the kernel: ``values`` returns the float64 image ``[3, H, W]`` of one frame's bytes, ``values32`` the
same formulas in float32, operation by operation, without fused multiply-add (what honest single-precision arithmetic gives; not a
model of the kernel).

The tolerance of tests/test_frames_in_gpu.py, |kernel - float64| <= TOL = 2^-20 on every element: ``values32`` against ``values``
over all 2^24 (y8, cb8, cr8) triples, both matrices and both ranges, differs by at most 2.2e-7 = 3.7 x 2^-24 after the clamp;
2^-20 is 4 x that and 1/4000 of a grey level.  The bilinear path interpolates exact codes (multiples of 1/16 below 256), so the
same bound holds for it.  tests/test_frames_in_cpu.py repeats the comparison on a subsample and asserts 2^-22."""
import numpy as np

MATRIX = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}
TOL = 2.0 ** -20


def frame_bytes(H, W, layout):
    return H * W * 3 // 2 if layout == "yuv420p" else 3 * H * W


def split(frame, H, W, layout):
    """One flat uint8 frame -> (rgb [H, W, 3],) or (y [H, W], u, v) with u, v [H, W] (yuv444p) or [H / 2, W / 2] (yuv420p)."""
    flat = np.asarray(frame, dtype=np.uint8).reshape(-1)
    assert flat.shape[0] == frame_bytes(H, W, layout), (flat.shape, H, W, layout)
    if layout == "rgb24":
        return (flat.reshape(H, W, 3),)
    ch, cw = (H // 2, W // 2) if layout == "yuv420p" else (H, W)
    return flat[:H * W].reshape(H, W), flat[H * W:H * W + ch * cw].reshape(ch, cw), flat[H * W + ch * cw:].reshape(ch, cw)


def _up_axis(c, axis, dtype):
    """One axis of the centre-sited 2x upsampling: position 2 j takes 0.25 c[j - 1] + 0.75 c[j], position 2 j + 1 takes
    0.75 c[j] + 0.25 c[j + 1], indices clamped."""
    c = np.moveaxis(c, axis, 0)
    n = c.shape[0]
    j = np.arange(n)
    left, right = c[np.maximum(j - 1, 0)], c[np.minimum(j + 1, n - 1)]
    q, t = dtype(0.25), dtype(0.75)
    out = np.empty((2 * n,) + c.shape[1:], dtype=dtype)
    out[0::2] = q * left + t * c
    out[1::2] = t * c + q * right
    return np.moveaxis(out, 0, axis)


def upsample_codes(c, chroma, dtype=np.float64):
    """A chroma plane of codes [H / 2, W / 2] -> [H, W]: ``nearest`` (each sample serves its 2x2 block) or ``bilinear``."""
    c = np.asarray(c).astype(dtype)
    if chroma == "nearest":
        return np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    assert chroma == "bilinear"
    return _up_axis(_up_axis(c, 1, dtype), 0, dtype)


def rgb_of_codes(y8, cb8, cr8, matrix="bt709", rng="limited", dtype=np.float64):
    """Codes (arrays of one shape; the chroma codes may be interpolated) -> [3, ...] R, G, B clamped to [0, 1].  ``dtype``
    float64: the reference.  float32: every constant rounded once to float32, every operation a float32 operation, no fused
    multiply-add."""
    f = dtype
    Kr, Kb = MATRIX[matrix]
    Kg = 1.0 - Kr - Kb
    r_cr, b_cb = f(2.0 * (1.0 - Kr)), f(2.0 * (1.0 - Kb))
    g_cr, g_cb = f(2.0 * Kr * (1.0 - Kr) / Kg), f(2.0 * Kb * (1.0 - Kb) / Kg)
    y8, cb8, cr8 = (np.asarray(v).astype(f) for v in (y8, cb8, cr8))
    if rng == "limited":
        Y, Cb, Cr = (y8 - f(16)) / f(219), (cb8 - f(128)) / f(224), (cr8 - f(128)) / f(224)
    else:
        assert rng == "full"
        Y, Cb, Cr = y8 / f(255), (cb8 - f(128)) / f(255), (cr8 - f(128)) / f(255)
    R = Y + r_cr * Cr
    B = Y + b_cb * Cb
    G = Y - g_cr * Cr - g_cb * Cb
    out = np.clip(np.stack([R, G, B]), f(0), f(1))
    assert out.dtype == f
    return out


def _image(frame, H, W, layout, matrix, rng, chroma, dtype):
    p = split(frame, H, W, layout)
    if layout == "rgb24":
        return np.transpose(p[0], (2, 0, 1)).astype(dtype) / dtype(255)
    y, u, v = p
    if layout == "yuv420p":
        u, v = upsample_codes(u, chroma, dtype), upsample_codes(v, chroma, dtype)
    return rgb_of_codes(y, u, v, matrix, rng, dtype)


def values(frame, H, W, layout, matrix="bt709", rng="limited", chroma="bilinear"):
    """One flat uint8 frame -> float64 [3, H, W]."""
    return _image(frame, H, W, layout, matrix, rng, chroma, np.float64)


def values32(frame, H, W, layout, matrix="bt709", rng="limited", chroma="bilinear"):
    out = _image(frame, H, W, layout, matrix, rng, chroma, np.float32)
    assert out.dtype == np.float32
    return out


def all_triples_frame():
    """The 4096 x 4096 yuv444p frame that holds every (y8, cb8, cr8) triple once: pixel p = 4096 row + column has y8 = p mod 256,
    cb8 = (p / 256) mod 256, cr8 = p / 65536."""
    p = np.arange(1 << 24, dtype=np.uint32)
    return np.concatenate([(p & 255).astype(np.uint8), ((p >> 8) & 255).astype(np.uint8), (p >> 16).astype(np.uint8)])


def random_frame(H, W, layout, seed):
    return np.random.default_rng(7000 + seed).integers(0, 256, frame_bytes(H, W, layout), dtype=np.uint8)


def checkerboard_frame(H, W, seed):
    """A yuv420p frame with random luma whose chroma planes are checkerboards of 0 and 255 (U and V in opposite phase): the worst
    case for a wrong neighbour or a wrong edge clamp — every neighbour differs by the full range."""
    y = np.random.default_rng(7100 + seed).integers(0, 256, H * W, dtype=np.uint8)
    i, j = np.meshgrid(np.arange(H // 2), np.arange(W // 2), indexing="ij")
    u = (((i + j) & 1) * 255).astype(np.uint8)
    return np.concatenate([y, u.reshape(-1), (255 - u).reshape(-1)])
