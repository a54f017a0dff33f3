"""float64 reference of the decoder's 8-bit output stage (numpy), written from the formulas of include/gsvc_hip.h, not from the
kernel: ``values`` returns the real-valued samples BEFORE rounding (what the tolerances of tests/test_frames_out_gpu.py are stated
on), ``convert`` the bytes an exact evaluation would give."""
import numpy as np

MATRIX = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}


def defaults(layout, rounding=None):
    return rounding if rounding is not None else ("trunc" if layout == "rgb24" else "nearest")


def values(img, layout, matrix="bt709", rng="limited"):
    """img [3, H, W] (any float dtype; NaN / inf allowed) -> flat float64 array of the frame's samples before rounding, already
    clamped to [0, 255], in the frame's byte order."""
    x = np.asarray(img, dtype=np.float64)
    c = np.where(x > 0, x, 0.0)          # NaN, -inf -> 0
    c = np.minimum(c, 1.0)               # +inf -> 1
    _, H, W = c.shape
    if layout == "rgb24":
        v = 255.0 * np.transpose(c, (1, 2, 0)).reshape(-1)
        return np.clip(v, 0.0, 255.0)
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
    if rng == "limited":
        y8, cb8, cr8 = 16.0 + 219.0 * Y, 128.0 + 224.0 * Cb, 128.0 + 224.0 * Cr
    else:
        assert rng == "full"
        y8, cb8, cr8 = 255.0 * Y, 128.0 + 255.0 * Cb, 128.0 + 255.0 * Cr
    return np.clip(np.concatenate([y8.reshape(-1), cb8.reshape(-1), cr8.reshape(-1)]), 0.0, 255.0)


def quantise(v, rounding):
    """(uint8) v  or  (uint8)(v + 0.5)  of values in [0, 255]."""
    if rounding == "trunc":
        return np.floor(v).astype(np.uint8)
    assert rounding == "nearest"
    return np.floor(v + 0.5).astype(np.uint8)


def convert(img, layout, matrix="bt709", rng="limited", rounding=None):
    return quantise(values(img, layout, matrix, rng), defaults(layout, rounding))


def check_bytes(got, v, rounding, delta=2.0 ** -11):
    """The issue's condition on every byte b against the float64 value v before rounding: nearest |b - v| <= 0.5 + delta; trunc
    v - 1 - delta < b <= v + delta.  Returns the number of bytes that break it and the worst excess."""
    b = np.asarray(got, dtype=np.float64).reshape(-1)
    assert b.shape == v.shape, (b.shape, v.shape)
    if rounding == "nearest":
        excess = np.abs(b - v) - (0.5 + delta)
        bad = excess > 0
    else:
        bad = ~((v - 1.0 - delta < b) & (b <= v + delta))
        excess = np.maximum(b - v - delta, v - 1.0 - delta - b)
    return int(bad.sum()), float(excess.max()) if excess.size else 0.0


def values32(img, layout, matrix="bt709", rng="limited"):
    """The same formulas evaluated in float32, operation by operation (no fused multiply-add, constants rounded to float32): what
    honest single-precision arithmetic gives.  Used to show that the tolerances above are loose for it; not a model of the kernel."""
    f = np.float32
    x = np.asarray(img, dtype=np.float32)
    c = np.minimum(np.where(x > 0, x, f(0)), f(1)).astype(np.float32)
    _, H, W = c.shape
    if layout == "rgb24":
        return np.clip(f(255) * np.transpose(c, (1, 2, 0)).reshape(-1), f(0), f(255))
    Kr, Kb = MATRIX[matrix]
    kr, kb, kg = f(Kr), f(Kb), f(1.0 - Kr - Kb)
    R, G, B = c
    Y = kr * R + kg * G + kb * B
    Cb = (B - Y) / f(2.0 * (1.0 - Kb))
    Cr = (R - Y) / f(2.0 * (1.0 - Kr))
    if layout == "yuv420p":
        Cb = Cb.reshape(H // 2, 2, W // 2, 2)
        Cb = ((Cb[:, 0, :, 0] + Cb[:, 0, :, 1]) + (Cb[:, 1, :, 0] + Cb[:, 1, :, 1])) * f(0.25)
        Cr = Cr.reshape(H // 2, 2, W // 2, 2)
        Cr = ((Cr[:, 0, :, 0] + Cr[:, 0, :, 1]) + (Cr[:, 1, :, 0] + Cr[:, 1, :, 1])) * f(0.25)
    if rng == "limited":
        y8, cb8, cr8 = f(16) + f(219) * Y, f(128) + f(224) * Cb, f(128) + f(224) * Cr
    else:
        y8, cb8, cr8 = f(255) * Y, f(128) + f(255) * Cb, f(128) + f(255) * Cr
    out = np.clip(np.concatenate([y8.reshape(-1), cb8.reshape(-1), cr8.reshape(-1)]), f(0), f(255))
    assert out.dtype == np.float32
    return out


def quantise32(v32, rounding):
    return np.floor(v32 + (np.float32(0.5) if rounding == "nearest" else np.float32(0.0))).astype(np.uint8)


KINDS = ("noise", "ramp", "k255", "special")


def make_image(kind, H, W, seed=0):
    """Seeded float32 [3, H, W] inputs of the conversion tests: uniform noise in [-0.1, 1.1]; a smooth ramp (a different surface
    per channel, a little outside [0, 1] at one end); exact k / 255 values; noise with a few NaN / +inf / -inf pixels."""
    rng = np.random.default_rng(1000 + seed)
    if kind == "noise" or kind == "special":
        img = rng.uniform(-0.1, 1.1, (3, H, W)).astype(np.float32)
        if kind == "special":
            flat = img.reshape(3, -1)
            n = max(3, min(12, H * W // 2))
            at = rng.choice(H * W, size=min(n, H * W), replace=False)
            for j, p in enumerate(at):
                flat[rng.integers(0, 3) if j % 2 else slice(None), p] = (np.nan, np.inf, -np.inf)[j % 3]
        return img
    if kind == "ramp":
        ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        u, v = xs / max(W - 1, 1), ys / max(H - 1, 1)
        # (no channel is constant along a row or a column: a value that happens to sit on a rounding tie is then not repeated H or W times)
        return np.stack([-0.02 + 1.04 * (0.7 * u + 0.3 * v), 0.9 - 0.85 * (0.35 * u + 0.65 * v * v), 0.1 + 0.4 * u * u + 0.45 * v]).astype(np.float32)
    assert kind == "k255"
    k = rng.integers(0, 256, (3, H, W)).astype(np.float32)
    return (k / np.float32(255.0)).astype(np.float32)
