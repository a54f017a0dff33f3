"""Plain statements of the spatially weighted distortion (csrc/wdist.hip, gsvc_amd/wdist.py), written from the definitions of DESIGN
section 8o.  The weighted SSIM / L1 is built on tests/_loss_kernel_refs.py (the window, the moments and the map are those of the unweighted
kernels) and is differentiable: called with float64 tensors it is the reference of tests/test_wdist_gpu.py, with float32 tensors "the fp32
tensor statement" those tests calibrate against.  The maps and the per-cell SSE are restated in numpy, pixel by pixel where the package
works on cells.  Nothing here imports the package under test.
"""
import numpy as np
import torch

from tests._loss_kernel_refs import ssim_map, ssim_moments


def map_shape(H, W, cell):
    return (H + cell - 1) // cell, (W + cell - 1) // cell


def pixel_weights(weights, cell, H, W):
    """[Hc, Wc] -> [H, W]: pixel (y, x) has weights[y // cell][x // cell] (an index per pixel, no reshaping)."""
    ys = torch.arange(H, device=weights.device) // cell
    xs = torch.arange(W, device=weights.device) // cell
    return weights[ys[:, None], xs[None, :]]


def wssim_l1_ref(img1, img2, weights, cell, w):
    """(sum w ssim_map, sum w |img1 - img2|) / (C H W) of two [C, H, W] images, in their dtype, differentiable."""
    C, H, W = img1.shape
    wp = pixel_weights(weights.to(img1.dtype), cell, H, W)
    n = C * H * W
    return (wp * ssim_map(*ssim_moments(img1, img2, w))).sum() / n, (wp * (img1 - img2).abs()).sum() / n


def wssim_l1_pair_ref(f, b, gt, weights, cell, w):
    return wssim_l1_ref((f + b.flip(-1)) / 2, gt, weights, cell, w)


def wssim_partials(img1, img2, weights, cell, w):
    """d (sum w map) / d (mu1, E[x^2], E[xy]) per pixel at fixed mu2 and E[y^2]: the maps the forward kernel stores."""
    C, H, W = img1.shape
    wp = pixel_weights(weights.to(img1.dtype), cell, H, W)
    mu1, mu2, e11, e22, e12 = (t.detach() for t in ssim_moments(img1.detach(), img2.detach(), w))
    mu1, e11, e12 = (t.clone().requires_grad_(True) for t in (mu1, e11, e12))
    return torch.autograd.grad((wp * ssim_map(mu1, mu2, e11, e22, e12)).sum(), (mu1, e11, e12))


# ------------------------------------------------------------------------------------------------------------ the maps (numpy, float64)
def pixels_of_cells(H, W, cell):
    """[Hc, Wc]: how many pixels of the picture each cell holds, counted pixel by pixel."""
    Hc, Wc = map_shape(H, W, cell)
    n = np.zeros((Hc, Wc), dtype=np.float64)
    for y in range(H):
        for x in range(W):
            n[y // cell, x // cell] += 1
    return n


def normalise_ref(maps, H, W, cell):
    m = np.asarray(maps, dtype=np.float64)
    n = pixels_of_cells(H, W, cell)
    out = np.empty_like(m)
    for t in range(m.shape[0]):
        out[t] = m[t] * (H * W / (m[t] * n).sum())
    return out.astype(np.float32)


def activity_weights_ref(dmap, H, W, cell, depth, strength, clamp):
    d = np.asarray(dmap).astype(np.float64)
    n = pixels_of_cells(H, W, cell)
    e = np.log2(1.0 + d / (n[None] * 2.0 ** (depth - 8)))
    mean_e = (e * n[None]).sum() / (d.shape[0] * H * W)
    w = np.minimum(np.maximum(np.exp2(-strength * (e - mean_e)), 1.0 / clamp), clamp)
    return normalise_ref(w, H, W, cell)


def roi_weights_ref(H, W, cell, rects, T):
    pix = np.ones((H, W), dtype=np.float64)
    for x, y, w, h, wt in rects:
        for yy in range(max(y, 0), min(y + h, H)):
            for xx in range(max(x, 0), min(x + w, W)):
                pix[yy, xx] = wt
    Hc, Wc = map_shape(H, W, cell)
    s = np.zeros((Hc, Wc), dtype=np.float64)
    for yy in range(H):
        for xx in range(W):
            s[yy // cell, xx // cell] += pix[yy, xx]
    return normalise_ref(np.repeat((s / pixels_of_cells(H, W, cell))[None], T, axis=0), H, W, cell)


def luma_codes(frames_u8, H, W, depth):
    """The luma plane of planar frames uint8 [n, >= frame bytes] -> int64 [n, H, W] (deep formats: little-endian 16-bit samples)."""
    f = np.asarray(frames_u8)
    if depth > 8:
        return np.ascontiguousarray(f[:, :2 * H * W]).view("<u2").astype(np.int64).reshape(-1, H, W)
    return f[:, :H * W].astype(np.int64).reshape(-1, H, W)


def block_sse_ref(a_u8, b_u8, H, W, depth, cell):
    """int64 [n, Hc, Wc]: squared luma code differences summed per cell."""
    d = (luma_codes(a_u8, H, W, depth) - luma_codes(b_u8, H, W, depth)) ** 2
    Hc, Wc = map_shape(H, W, cell)
    pad = np.zeros((d.shape[0], Hc * cell, Wc * cell), dtype=np.int64)
    pad[:, :H, :W] = d
    return pad.reshape(-1, Hc, cell, Wc, cell).sum(axis=(2, 4))


def weighted_psnr_y_ref(sse, weights, depth, H, W):
    sse, w = np.asarray(sse, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    peak2 = float((1 << depth) - 1) ** 2
    per = np.array([10.0 * np.log10(peak2 * H * W / (w[t] * sse[t]).sum()) for t in range(sse.shape[0])])
    return per, 10.0 * np.log10(peak2 * H * W * sse.shape[0] / (w * sse).sum())
