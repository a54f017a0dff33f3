"""References of the MS-SSIM + L1 loss (csrc/msssim_loss.hip): MS-SSIM restated in tensor expressions of the inputs' own dtype (float64:
the reference; float32: the yardstick whose error the kernels are measured against), the backward formula written out by hand in
float64 without autograd, and the test pictures.

The function: per plane of ``[P, H, W]``, five scales; per scale the VALID blur with the normalised 11-tap Gaussian (sigma 1.5) of
x, y, x^2, y^2, xy, the mean t_s of the contrast-structure map (s < 4) or of the SSIM map (s = 4); between scales the 2x2 mean with a
leading zero row / column on an odd side; v = prod relu(t_s)^w_s; the value is the mean of v over the planes."""
import torch
import torch.nn.functional as F

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C1, C2 = 0.01 ** 2, 0.03 ** 2
TAPS = 11
SHAPES = [(161, 161, 1), (170, 202, 3), (176, 208, 2), (193, 163, 1)]
SHAPE_IDS = [f"{h}x{w}x{p}" for h, w, p in SHAPES]
SIGMAS = (0.02, 0.1)


def window(dtype, device):
    x = torch.arange(TAPS, dtype=torch.float64) - TAPS // 2
    g = torch.exp(-(x ** 2) / (2 * 1.5 ** 2))
    return (g / g.sum()).to(device=device, dtype=dtype)


def blur(x, w):
    """VALID separable blur of [P, h, w] planes, along H then W."""
    x = F.conv2d(x.unsqueeze(1), w.view(1, 1, -1, 1))
    return F.conv2d(x, w.view(1, 1, 1, -1)).squeeze(1)


def pool(x):
    """2x2 mean; an odd side gets one leading zero row / column and the divisor stays 4."""
    return F.avg_pool2d(x.unsqueeze(1), kernel_size=2, padding=[x.shape[1] % 2, x.shape[2] % 2]).squeeze(1)


def scale_maps(x, y, w, last):
    mu1, mu2 = blur(x, w), blur(y, w)
    s1 = blur(x * x, w) - mu1 * mu1
    s2 = blur(y * y, w) - mu2 * mu2
    s12 = blur(x * y, w) - mu1 * mu2
    cs = (2 * s12 + C2) / (s1 + s2 + C2)
    if not last:
        return cs
    return (2 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs


def ms_terms(x, y):
    """[5, P] per-scale means in the dtype of x."""
    w = window(x.dtype, x.device)
    t = []
    for s in range(5):
        t.append(scale_maps(x, y, w, s == 4).flatten(1).mean(1))
        if s < 4:
            x, y = pool(x), pool(y)
    return torch.stack(t)


def ms_value(t):
    wts = torch.tensor(MS_WEIGHTS, dtype=t.dtype, device=t.device).view(-1, 1)
    return torch.prod(torch.relu(t) ** wts, dim=0)


def ms_ssim_l1(x, y):
    """(MS-SSIM, L1) of [P, H, W] planes in their own dtype; differentiable."""
    return ms_value(ms_terms(x, y)).mean(), (x - y).abs().mean()


def grad_autograd(x, y, g_ms, g_l1):
    x = x.detach().clone().requires_grad_(True)
    ms, l1 = ms_ssim_l1(x, y)
    (g_ms * ms + g_l1 * l1).backward()
    return x.grad.detach()


# ------------------------------------------------------------------------------------------------ the backward by hand
def _blur_adjoint(m, w):
    """Gt: the valid blur's adjoint = the same (symmetric) blur of the map extended by 10 zeros on every side."""
    return blur(F.pad(m, (TAPS - 1,) * 4), w)


def _pool_adjoint(d, h, w):
    """Pt: 0.25 * D((r + h % 2) // 2, (c + w % 2) // 2) for the h x w inputs."""
    r = (torch.arange(h, device=d.device) + h % 2) // 2
    c = (torch.arange(w, device=d.device) + w % 2) // 2
    return 0.25 * d[:, r][:, :, c]


def grad_by_hand(x, y, g_ms, g_l1):
    """The gradient of g_ms * MS-SSIM + g_l1 * L1 with respect to x, float64, no autograd: scale 4 down to scale 0,
    D_s = (g w_s v / t_s / n_s / P) [Gt(dM/dmu1) + 2 X_s Gt(dM/dE11) + Y_s Gt(dM/dE12)] + Pt D_{s+1}, + g_l1 / (P H W) sign(x - y)."""
    assert x.dtype == torch.float64
    P, H, W = x.shape
    w = window(x.dtype, x.device)
    xs, ys = [x], [y]
    for _ in range(4):
        xs.append(pool(xs[-1]))
        ys.append(pool(ys[-1]))
    parts, t = [], []
    for s in range(5):
        X, Y = xs[s], ys[s]
        mu1, mu2 = blur(X, w), blur(Y, w)
        s1, s2, s12 = blur(X * X, w) - mu1 * mu1, blur(Y * Y, w) - mu2 * mu2, blur(X * Y, w) - mu1 * mu2
        den = s1 + s2 + C2
        cs = (2 * s12 + C2) / den
        dB, dC = -cs / den, 2 / den                       # d cs / d E11, d cs / d E12
        dA = -(2 * mu1 * dB + mu2 * dC)                   # d cs / d mu1 (through sigma1^2 and sigma12)
        M = cs
        if s == 4:
            la = mu1 * mu1 + mu2 * mu2 + C1
            lum = (2 * mu1 * mu2 + C1) / la
            dlum = 2 * (mu2 - lum * mu1) / la
            M = lum * cs
            dA, dB, dC = cs * dlum + lum * dA, lum * dB, lum * dC
        t.append(M.flatten(1).mean(1))
        parts.append((dA, dB, dC, M.shape[1] * M.shape[2]))
    t = torch.stack(t)
    clipped = (t <= 0).any(0)
    v = ms_value(t)
    D = None
    for s in range(4, -1, -1):
        dA, dB, dC, n = parts[s]
        k = g_ms * MS_WEIGHTS[s] * v / t[s] / n / P
        k = torch.where(clipped, torch.zeros_like(k), k).view(-1, 1, 1)
        d = k * (_blur_adjoint(dA, w) + 2 * xs[s] * _blur_adjoint(dB, w) + ys[s] * _blur_adjoint(dC, w))
        if D is not None:
            d = d + _pool_adjoint(D, xs[s].shape[1], xs[s].shape[2])
        D = d
    return D + g_l1 / (P * H * W) * torch.sign(x - y)


# ------------------------------------------------------------------------------------------------ the test pictures
def pictures(H, W, P, sigma, seed=0, device="cpu"):
    """(x, y) float64 [P, H, W]: y a bicubic upsampling of uniform noise of (H/8 + 2) x (W/8 + 2) plus 0.05 uniform, clamped; x = y plus
    Gaussian noise of the given sigma, clamped."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + P)
    low = torch.rand((1, P, H // 8 + 2, W // 8 + 2), generator=g, dtype=torch.float64)
    y = F.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)[0]
    y = (y + 0.05 * torch.rand((P, H, W), generator=g, dtype=torch.float64)).clamp(0, 1)
    x = (y + sigma * torch.randn((P, H, W), generator=g, dtype=torch.float64)).clamp(0, 1)
    return x.to(device), y.to(device)
