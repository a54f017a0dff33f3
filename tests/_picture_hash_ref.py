"""NumPy statement of the picture hash (include/gsvc_hip.h, gsvc_picture_hash; the PHSH section of a bitstream file): for plane p of a
frame, s the 0-based raster index of a sample within its plane (rgb24: plane = channel, s = the pixel index), c its code, in uint32:

    x  = s * 0x9E3779B1  ^  (c + 1) * 0x85EBCA6B
    x ^= x >> 15;  x *= 0x2C1B3C6D;  x ^= x >> 12
    hash[p] = the sum of x over the plane, modulo 2^64

uint32 arrays wrap on multiplication, uint64 sums wrap on overflow: nothing here is a float."""
import numpy as np

M1, M2, M3 = np.uint32(0x9E3779B1), np.uint32(0x85EBCA6B), np.uint32(0x2C1B3C6D)


def mix(s, c):
    """uint32 arrays (positions, codes) -> uint32 array."""
    s, c = np.asarray(s).astype(np.uint32), np.asarray(c).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = (s * M1) ^ ((c + np.uint32(1)) * M2)
        x ^= x >> np.uint32(15)
        x = x * M3
        x ^= x >> np.uint32(12)
    return x


def plane_hash(codes) -> int:
    """The hash of one plane: its codes in raster order (any integer array) -> a Python int below 2^64."""
    codes = np.asarray(codes).reshape(-1)
    x = mix(np.arange(codes.size, dtype=np.uint64), codes)
    return int(x.astype(np.uint64).sum(dtype=np.uint64))


def frame_planes(frame_u8, H, W, layout, depth):
    """One flat frame (uint8, at least frame_bytes long) -> its three planes' codes in raster order."""
    per = 2 if depth > 8 else 1
    px = H * W
    samples = px * 3 // 2 if layout == "yuv420p" else 3 * px
    codes = np.ascontiguousarray(np.asarray(frame_u8).reshape(-1)[:samples * per]).view("<u2" if per == 2 else np.uint8)
    if layout == "rgb24":
        rgb = codes.reshape(px, 3)
        return [rgb[:, 0], rgb[:, 1], rgb[:, 2]]
    ch = px // 4 if layout == "yuv420p" else px
    return [codes[:px], codes[px:px + ch], codes[px + ch:px + 2 * ch]]


def picture_hash_ref(frames_u8, H, W, layout, depth):
    """uint8 [n, >= frame_bytes] -> uint64 [n, 3]."""
    frames_u8 = np.asarray(frames_u8)
    out = np.zeros((frames_u8.shape[0], 3), np.uint64)
    for k in range(frames_u8.shape[0]):
        out[k] = [plane_hash(p) for p in frame_planes(frames_u8[k], H, W, layout, depth)]
    return out
