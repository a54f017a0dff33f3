"""Plain statements of csrc/yuv_loss.hip, written from the formulas of include/gsvc_hip.h and not from the kernels: the Y'CbCr plane
transform of a render and its adjoint as tensor expressions (float64 tensors give the reference, float32 tensors "the fp32 tensor
statement" the GPU tests calibrate against), the planes of a file's sample codes as a numpy float32 restatement (that kernel is bit
exact), and the loss built from them with the SSIM reference of tests/_loss_kernel_refs.py.  tests/test_yuv_loss_cpu.py pins them
without a GPU.  Nothing here imports the package under test.
"""
import numpy as np
import torch

from tests._loss_kernel_refs import ssim_l1_ref

MATRIX = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}
LAYOUT_ID = {"rgb24": 0, "yuv444p": 1, "yuv420p": 2}
MATRIX_ID = {"bt709": 0, "bt601": 1}
RANGE_ID = {"limited": 0, "full": 1}


def chroma_size(H, W, layout):
    return (H // 2, W // 2) if layout == "yuv420p" else (H, W)


def plane_floats(H, W, layout):
    ch, cw = chroma_size(H, W, layout)
    return H * W + 2 * ch * cw


def constants(matrix, dtype):
    """(Kr, Kg, Kb, s_b, s_r) formed in double and rounded once to ``dtype`` (float64: not rounded)."""
    Kr, Kb = MATRIX[matrix]
    vals = (Kr, 1.0 - Kr - Kb, Kb, 1.0 / (2.0 * (1.0 - Kb)), 1.0 / (2.0 * (1.0 - Kr)))
    if dtype == torch.float32:
        return tuple(float(np.float32(v)) for v in vals)
    return vals


def two_view(f, b=None):
    """a = 0.5 (f + flip_W(b)); a = f without b."""
    return f if b is None else 0.5 * (f + b.flip(-1))


def planes_ref(f, b, layout, matrix):
    """(planes [H W + 2 ch cw], a [3, H, W]) of [3, H, W] images in their dtype; differentiable."""
    a = two_view(f, b)
    _, H, W = a.shape
    kr, kg, kb, sb, sr = constants(matrix, a.dtype)
    R, G, B = a[0], a[1], a[2]
    Y = kr * R + (kg * G + kb * B)
    Cb = (B - Y) * sb + 0.5
    Cr = (R - Y) * sr + 0.5
    if layout == "yuv420p":
        assert H % 2 == 0 and W % 2 == 0

        def mean(c):
            c = c.reshape(H // 2, 2, W // 2, 2)
            return 0.25 * ((c[:, 0, :, 0] + c[:, 0, :, 1]) + (c[:, 1, :, 0] + c[:, 1, :, 1]))
        Cb, Cr = mean(Cb), mean(Cr)
    else:
        assert layout == "yuv444p"
    return torch.cat([Y.reshape(-1), Cb.reshape(-1), Cr.reshape(-1)]), a


def split(planes, H, W, layout):
    """(Y [1, H, W], C [2, ch, cw]) of a flat plane buffer."""
    ch, cw = chroma_size(H, W, layout)
    return planes[:H * W].reshape(1, H, W), planes[H * W:H * W + 2 * ch * cw].reshape(2, ch, cw)


def adjoint_ref(g, H, W, layout, matrix, pair):
    """The adjoint of planes_ref's linear part, by its own formulas: g = (gY, gCb, gCr) in the plane layout -> (d_f, d_b or None)."""
    kr, kg, kb, sb, sr = constants(matrix, g.dtype)
    gY, gC = split(g, H, W, layout)
    gY, gCb, gCr = gY[0], gC[0], gC[1]
    q = 1.0
    if layout == "yuv420p":
        q = 0.25
        gCb = gCb.repeat_interleave(2, 0).repeat_interleave(2, 1)
        gCr = gCr.repeat_interleave(2, 0).repeat_interleave(2, 1)
    gB = q * gCb * sb
    gR = q * gCr * sr
    gYp = gY - gB - gR
    d = torch.stack([kr * gYp + gR, kg * gYp, kb * gYp + gB])
    if not pair:
        return d, None
    return 0.5 * d, (0.5 * d).flip(-1)


def yuv_ssim_l1_ref(f, b, tY, tC, layout, matrix, w):
    """(ssim_y, l1_y, ssim_c, l1_c) of the render's planes against the target planes; differentiable."""
    planes, _ = planes_ref(f, b, layout, matrix)
    Y, C = split(planes, f.shape[1], f.shape[2], layout)
    return ssim_l1_ref(Y, tY, w) + ssim_l1_ref(C, tC, w)


# ------------------------------------------------------------------------------------------------------------ sample codes
def range_constants(rng, depth):
    """(y_off, y_scale, c_off, c_scale, top) of a range at a depth (include/gsvc_hip.h)."""
    up, top = float(1 << (depth - 8)), float((1 << depth) - 1)
    if rng == "limited":
        return 16.0 * up, 219.0 * up, 128.0 * up, 224.0 * up, top
    assert rng == "full"
    return 0.0, top, 128.0 * up, top, top


def code_planes_ref(codes, H, W, rng, depth):
    """numpy: the flat sample codes of one planar frame (any integer dtype) -> float32 planes, operation by operation in float32:
    Y = (y - y_off) / y_scale, C = (c - c_off) / c_scale + 0.5."""
    f = np.float32
    y_off, y_scale, c_off, c_scale, _ = range_constants(rng, depth)
    c = np.asarray(codes).astype(np.float32)
    out = np.empty(c.shape, np.float32)
    n = H * W
    out[:n] = (c[:n] - f(y_off)) / f(y_scale)
    out[n:] = (c[n:] - f(c_off)) / f(c_scale) + f(0.5)
    assert out.dtype == np.float32
    return out


def codes_of_planes(planes, H, W, rng, depth=8):
    """What separates the planes from a delivered frame: clamp, range map and rounding to nearest.  Returns (codes, values before
    rounding) as float64 numpy arrays in the frame's sample order."""
    y_off, y_scale, c_off, c_scale, top = range_constants(rng, depth)
    p = np.asarray(planes, dtype=np.float64)
    n = H * W
    v = np.concatenate([y_off + y_scale * p[:n], c_off + c_scale * (p[n:] - 0.5)])
    v = np.clip(v, 0.0, top)
    return np.floor(v + 0.5), v


def make_codes(H, W, layout, depth, seed, n=1):
    """Seeded sample codes [n, samples] over the whole code range of a depth (the ends included), as uint8 or uint16."""
    rng = np.random.default_rng(4000 + seed)
    samples = plane_floats(H, W, layout)
    top = (1 << depth) - 1
    c = rng.integers(0, top + 1, (n, samples))
    c[:, 0], c[:, -1] = 0, top
    return c.astype(np.uint8 if depth == 8 else np.uint16)
