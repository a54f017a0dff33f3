"""Plain tensor statements of the kernels behind the loss value and the first gradients of a fitting step, written from the
kernels' header comments (csrc/ssim.hip, csrc/losses.hip, csrc/rate.hip k_rate_fwd / k_rate_bwd, the noise quantiser of
csrc/quant.hip).  Called with float64 tensors they are the references of tests/test_loss_kernels_gpu.py; called with float32
tensors they are "the fp32 tensor statement" those tests calibrate against.  tests/test_loss_kernel_refs_cpu.py pins them without a
GPU.  Nothing here imports the package under test.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests._step_kernel_refs import EPS32, PRINT, err, err_each, ulp_distance  # noqa: F401  (re-exported for the tests)

SSIM_C1, SSIM_C2 = 0.01 ** 2, 0.03 ** 2
LOW_BOUND = 2.0 ** -16
CLAMP_STEPS = 15000.0


# ------------------------------------------------------------------------------------------------------------ SSIM / L1
def ssim_window():
    """The eleven fp32 taps as make_loss_window() of csrc/ssim_tile.h builds them: exp(-(i - 5)^2 / (2 * 1.5^2)) in double, each tap rounded
    to float, divided by the float sum (the rounded taps added one by one in float, in tap order).  The taps are an input of the
    operation: a float64 reference uses these fp32 values cast up."""
    g = [np.float32(math.exp(-float((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5))) for i in range(11)]
    s = np.float32(0.0)
    for v in g:
        s = np.float32(s + v)
    return torch.from_numpy(np.array([np.float32(v / s) for v in g], dtype=np.float32))


def _blur11(x, w):
    """Zero-padded 11-tap blur of the last two dimensions, along the rows first and then along the columns, each as eleven shifted
    slices of the padded tensor times the taps, added in tap order."""
    H, W = x.shape[-2:]
    p = F.pad(x, (5, 5, 0, 0))
    h = sum(w[k] * p[..., :, k:k + W] for k in range(11))
    p = F.pad(h, (0, 0, 5, 5))
    return sum(w[k] * p[..., k:k + H, :] for k in range(11))


def ssim_moments(img1, img2, w):
    """(mu1, mu2, E[x^2], E[y^2], E[xy]): the blurred images and the blurred products (products formed before blurring)."""
    w = w.to(device=img1.device, dtype=img1.dtype)
    return tuple(_blur11(t, w) for t in (img1, img2, img1 * img1, img2 * img2, img1 * img2))


def ssim_map(mu1, mu2, e11, e22, e12):
    """The SSIM map as a function of the five moments (sigma1^2 = E[x^2] - mu1^2, sigma12 = E[xy] - mu1 mu2)."""
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
    return ((2 * mu12 + SSIM_C1) * (2 * s12 + SSIM_C2)) / ((mu1_sq + mu2_sq + SSIM_C1) * (s1 + s2 + SSIM_C2))


def ssim_partials(img1, img2, w):
    """d map / d (mu1, E[x^2], E[xy]) per pixel at fixed mu2 and E[y^2], by autograd in the dtype of the images."""
    mu1, mu2, e11, e22, e12 = (t.detach() for t in ssim_moments(img1.detach(), img2.detach(), w))
    mu1, e11, e12 = (t.clone().requires_grad_(True) for t in (mu1, e11, e12))
    return torch.autograd.grad(ssim_map(mu1, mu2, e11, e22, e12).sum(), (mu1, e11, e12))


def ssim_l1_ref(img1, img2, w):
    """(mean of the SSIM map, mean |img1 - img2|) of two [C, H, W] images, differentiable."""
    return ssim_map(*ssim_moments(img1, img2, w)).mean(), (img1 - img2).abs().mean()


def ssim_l1_pair_ref(f, b, gt, w):
    """The same on the two-view frame (f + flip_W(b)) / 2."""
    return ssim_l1_ref((f + b.flip(-1)) / 2, gt, w)


# ------------------------------------------------------------------------------------------------------------ regularisers
def regs_ref(scaling, opacity, mask, offs):
    """(sum_r mean over the masked Gaussians of render r of prod_c scaling, sum_r mean over render r of (1 - opacity)) for renders
    [offs[r], offs[r + 1]); empty renders are skipped, a render with nothing masked gives 0 / 0 = nan like the mean of an empty
    selection."""
    a = b = None
    m = mask.to(scaling.dtype)
    for lo, hi in zip(offs[:-1], offs[1:]):
        if hi <= lo:
            continue
        ta = (scaling[lo:hi].prod(1) * m[lo:hi]).sum() / m[lo:hi].sum()
        tb = (1 - opacity.reshape(-1)[lo:hi]).mean()
        a, b = (ta, tb) if a is None else (a + ta, b + tb)
    return a, b


# ------------------------------------------------------------------------------------------------------------ optical flow
def optical_pair_ref(world1, mask1, vis1, world2, mask2, vis2, flow, K, x_min, y_min, scale, x_pix_max, y_pix_max):
    """Optical-flow consistency of one pair of un-compacted renders.  Gaussian i of a render is slot i % K of anchor vis[i // K];
    the Gaussians masked in both renders with the same (anchor, slot) are paired; a pair counts iff the pixel of its first
    Gaussian, torch.round of the FP32 product (xy - min) * scale whatever dtype the errors are summed in (the decision is part
    of the operation), satisfies 0 <= p < pix_max.  flow [2, h, w] is read at [c, py, px] and divided by scale.
    Returns (loss = sum(|ex| + |ey|) / (2 n), n, (s1 [n1, 2], s2 [n2, 2])): s = d loss / d world[:, :2] * (2 n), in {-1, 0, 1}."""
    dt, dev = world1.dtype, world1.device
    n1, n2 = world1.shape[0], world2.shape[0]
    s1, s2 = torch.zeros(n1, 2, dtype=dt, device=dev), torch.zeros(n2, 2, dtype=dt, device=dev)
    zero = torch.zeros((), dtype=dt, device=dev)
    if n1 == 0 or n2 == 0:
        return zero, 0, (s1, s2)
    slot1, slot2 = torch.arange(n1, device=dev) % K, torch.arange(n2, device=dev) % K
    key1 = vis1.repeat_interleave(K) * K + slot1
    key2 = vis2.repeat_interleave(K) * K + slot2
    i2 = mask2.nonzero().squeeze(1)
    if i2.numel() == 0:
        return zero, 0, (s1, s2)
    k2, order = torch.sort(key2[i2])
    pos = torch.searchsorted(k2, key1).clamp_max(k2.numel() - 1)
    hit = mask1 & (k2[pos] == key1)
    partner = i2[order][pos]
    f32 = torch.float32
    lo32 = torch.tensor([x_min, y_min], dtype=f32, device=dev)
    pix = ((world1[:, :2].to(f32) - lo32) * torch.tensor(scale, dtype=f32, device=dev)).round()
    ok = hit & (pix[:, 0] >= 0) & (pix[:, 1] >= 0) & (pix[:, 0] < x_pix_max) & (pix[:, 1] < y_pix_max)
    i1 = ok.nonzero().squeeze(1)
    n = int(i1.numel())
    if n == 0:
        return zero, 0, (s1, s2)
    px, py = pix[i1, 0].long(), pix[i1, 1].long()
    uv = flow.to(dt)[:, py, px].t() / scale
    j = partner[i1]
    e = (world2[j, :2] - world1[i1, :2]) - uv
    loss = e.abs().sum() / (2 * n)
    sg = torch.sign(e.detach())
    s1[i1] = -sg
    s2[j] = sg
    return loss, n, (s1, s2)


# ------------------------------------------------------------------------------------------------------------ rate
def rate_bits_ref(x, mean, scale, q_rows, lo, hi):
    """bits = -log2 max(Phi((xc + Q/2 - mean) / scale) - Phi((xc - Q/2 - mean) / scale), 2^-16), xc = clamp(x, lo, hi), for x [n, c];
    q_rows: [n] tensor (or [n, c]: a copy of Q per element, whose gradient holds the terms of dQ's row sums) or a number; lo, hi: numbers or [n] tensors (per-row bounds).  Returns (bits, the unfloored likelihood).
    Under autograd the net Low_bound rule holds (no gradient where the unfloored likelihood is below 2^-16) and dx passes where
    lo <= x <= hi, equality included."""
    dt, dev = x.dtype, x.device
    t = lambda v: ((v if v.dim() == 2 else v.reshape(-1, 1)).to(dt) if torch.is_tensor(v) else torch.tensor(float(v), dtype=dt, device=dev))  # noqa: E731
    q, lo, hi = t(q_rows), t(lo), t(hi)
    inside = (x >= lo) & (x <= hi)
    xc = torch.where(inside, x, torch.minimum(torch.maximum(x.detach(), lo), hi))
    upper = torch.special.ndtr((xc + 0.5 * q - mean) / scale)
    lower = torch.special.ndtr((xc - 0.5 * q - mean) / scale)
    raw = upper - lower
    lik = torch.where(raw >= LOW_BOUND, raw, torch.full_like(raw, LOW_BOUND).detach())
    return -torch.log2(lik), raw


# ------------------------------------------------------------------------------------------------------------ noise quantiser
def _row_render(offs, rows, dev):
    r = torch.zeros(rows, dtype=torch.long, device=dev)
    for i, (lo, hi) in enumerate(zip(offs[:-1], offs[1:])):
        r[lo:hi] = i
    return r


def noise_quant_ref(x, q, noise, offs):
    """y = clamp(x / Q, c_r - 15000, c_r + 15000) * Q + noise * Q for x [rows, C] in renders [offs[r], offs[r + 1]) of rows, with
    centre c_r = mean(x over render r) / mean(Q over render r) (no gradient); q: [rows] tensor, or a number or 0-dim tensor.
    Returns (y, centre [R] (nan for an empty render), inside [rows, C]: the clamp is inactive)."""
    dt, dev = x.dtype, x.device
    R = len(offs) - 1
    per_row = torch.is_tensor(q) and q.dim() > 0
    Q = q.to(dt).reshape(-1, 1) if per_row else torch.as_tensor(q, dtype=dt, device=dev)
    centre = torch.full((R,), float("nan"), dtype=dt, device=dev)
    for r, (lo, hi) in enumerate(zip(offs[:-1], offs[1:])):
        if hi > lo:
            centre[r] = x[lo:hi].detach().mean() / (Q[lo:hi].detach().mean() if per_row else Q.detach())
    c = centre[_row_render(offs, x.shape[0], dev)].reshape(-1, 1)
    v = x / Q
    inside = (v >= c - CLAMP_STEPS) & (v <= c + CLAMP_STEPS)
    y = torch.minimum(torch.maximum(v, c - CLAMP_STEPS), c + CLAMP_STEPS) * Q + noise * Q
    return y, centre, inside.detach()


def noise_quant_grads(g, x, q, noise, offs):
    """The analytic gradients of noise_quant_ref for upstream g: dx = g * inside, dq[row] = sum_c g * ((inside ? 0 : clamped value)
    + noise); also returns sum_c |g * term|, the scale dq is compared on."""
    dt, dev = x.dtype, x.device
    _, centre, inside = noise_quant_ref(x, q, noise, offs)
    Q = q.to(dt).reshape(-1, 1) if torch.is_tensor(q) and q.dim() > 0 else torch.as_tensor(q, dtype=dt, device=dev)
    c = centre[_row_render(offs, x.shape[0], dev)].reshape(-1, 1)
    clamped = torch.minimum(torch.maximum(x / Q, c - CLAMP_STEPS), c + CLAMP_STEPS)
    term = torch.where(inside, torch.zeros_like(clamped), clamped) + noise
    return g * inside, (g * term).sum(1), (g * term).abs().sum(1)
