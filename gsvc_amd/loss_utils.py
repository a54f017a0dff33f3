"""Losses of the fitting step: L1, SSIM (11x11 Gaussian window, sigma 1.5, zero padding), optical-flow
consistency of Gaussian motion between adjacent frames.

Same values as reference utils/loss_utils.py:20-72 (l1_loss_func, ssim_func/_ssim) and :76-153
(calc_optical_loss_one_frame / calc_optical_loss).  SSIM uses the separability of the window (two 1-D
passes instead of one 11x11 depthwise conv per moment) and filters the five moments in one batched call.
"""
from __future__ import annotations

from functools import lru_cache
from math import exp

import torch
import torch.nn.functional as F

from . import yuv_loss


class _SsimL1(torch.autograd.Function):
    """(mean SSIM, mean |x - gt|[, x]) of [C,H,W] CUDA images through csrc/ssim.hip; ``img_b`` not None is the pair form
    x = (img + flip_W(img_b)) / 2 formed inside the kernels (the two-view frame of reference pipeline/train.py:368-375: no flip / add /
    div launches forward, no div / flip backward), and x is the third result (non-differentiable)."""

    @staticmethod
    def forward(ctx, img, img_b, gt):
        from . import _lib
        pair = img_b is not None
        a, g = img.contiguous().float(), gt.contiguous().float()
        b = img_b.contiguous().float() if pair else None
        C_, H, W = a.shape
        need = img.requires_grad or (pair and img_b.requires_grad)
        sums = torch.empty(2, device=a.device, dtype=torch.float32)
        work = torch.empty(2048, device=a.device, dtype=torch.float32)
        avg = torch.empty_like(a) if pair else None
        maps = [torch.empty_like(a) for _ in range(3)] if need else [None, None, None]
        L, st = _lib.lib(), _lib.current_stream(a.device)
        if pair:
            _lib.check(L.gsvc_ssim_l1_pair_forward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(g), C_, H, W, _lib.ptr(sums), _lib.ptr(work),
                                                   _lib.ptr(maps[0]), _lib.ptr(maps[1]), _lib.ptr(maps[2]), _lib.ptr(avg), st),
                       "gsvc_ssim_l1_pair_forward")
        else:
            _lib.check(L.gsvc_ssim_l1_forward(_lib.ptr(a), _lib.ptr(g), C_, H, W, _lib.ptr(sums), _lib.ptr(work), _lib.ptr(maps[0]),
                                              _lib.ptr(maps[1]), _lib.ptr(maps[2]), st), "gsvc_ssim_l1_forward")
        if need:
            ctx.save_for_backward(a, g, *maps, *((b,) if pair else ()))
        ctx.pair = pair
        ctx.set_materialize_grads(False)      # no zero image for the averaged frame's (absent) gradient
        out = sums / float(C_ * H * W)
        if pair:
            ctx.mark_non_differentiable(avg)
            return out[0], out[1], avg
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_ssim, g_l1, _g_avg=None):
        from . import _lib
        a, g, m0, m1, m2 = ctx.saved_tensors[:5]
        b = ctx.saved_tensors[5] if ctx.pair else None
        C_, H, W = a.shape
        zero = torch.zeros((), device=a.device) if (g_ssim is None or g_l1 is None) else None
        grads = torch.stack([zero if g_ssim is None else g_ssim, zero if g_l1 is None else g_l1]).float().contiguous()
        d = torch.empty_like(a)
        db = torch.empty_like(b) if ctx.pair else None
        L, st = _lib.lib(), _lib.current_stream(a.device)
        if ctx.pair:
            _lib.check(L.gsvc_ssim_l1_pair_backward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(g), C_, H, W, _lib.ptr(grads), _lib.ptr(m0),
                                                    _lib.ptr(m1), _lib.ptr(m2), _lib.ptr(d), _lib.ptr(db), st), "gsvc_ssim_l1_pair_backward")
        else:
            _lib.check(L.gsvc_ssim_l1_backward(_lib.ptr(a), _lib.ptr(g), C_, H, W, _lib.ptr(grads), _lib.ptr(m0), _lib.ptr(m1),
                                               _lib.ptr(m2), _lib.ptr(d), st), "gsvc_ssim_l1_backward")
        return d, db, None


def ssim_l1(img, gt, img_b=None):
    """Fused (ssim_func(x, gt), l1_loss_func(x, gt)) for [C,H,W] CUDA images (one kernel each way); the gradient goes to ``img`` (and
    ``img_b``).  x = img, or with ``img_b`` the two-view frame x = (img + flip(img_b, W)) / 2, then also returned, detached, as a third
    result."""
    return _SsimL1.apply(img, img_b, gt)


class _MsSsimL1(torch.autograd.Function):
    """(MS-SSIM, mean |x - gt|[, x]) of [C,H,W] CUDA images through csrc/msssim_loss.hip; ``img_b`` not None is the pair form
    x = (img + flip_W(img_b)) / 2, formed inside the kernels, and x is the third result (non-differentiable)."""

    @staticmethod
    def forward(ctx, img, img_b, gt):
        from . import _lib
        pair = img_b is not None
        a, g = img.contiguous().float(), gt.contiguous().float()
        b = img_b.contiguous().float() if pair else None
        C_, H, W = a.shape
        L = _lib.lib()
        nbytes = int(L.gsvc_msssim_loss_workspace_bytes(C_, H, W))
        if nbytes < 0:
            raise ValueError(f"ms_ssim_l1: image sides must exceed 160 pixels for 5 scales (got {C_} planes of {H} x {W})")
        need = img.requires_grad or (pair and img_b.requires_grad)
        work = torch.empty(nbytes, device=a.device, dtype=torch.uint8)
        out = torch.empty(2, device=a.device, dtype=torch.float32)
        avg = torch.empty_like(a) if pair else None
        _lib.check(L.gsvc_msssim_loss_forward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(g), C_, H, W, int(need), _lib.ptr(work), _lib.ptr(out),
                                              _lib.ptr(avg), _lib.current_stream(a.device)), "gsvc_msssim_loss_forward")
        if need:
            ctx.save_for_backward(a, g, work, *((b,) if pair else ()))
        ctx.pair = pair
        ctx.set_materialize_grads(False)
        if pair:
            ctx.mark_non_differentiable(avg)
            return out[0], out[1], avg
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_ms, g_l1, _g_avg=None):
        from . import _lib
        a, g, work = ctx.saved_tensors[:3]
        b = ctx.saved_tensors[3] if ctx.pair else None
        C_, H, W = a.shape
        zero = torch.zeros((), device=a.device) if (g_ms is None or g_l1 is None) else None
        grads = torch.stack([zero if g_ms is None else g_ms, zero if g_l1 is None else g_l1]).float().contiguous()
        d = torch.empty_like(a)
        db = torch.empty_like(b) if ctx.pair else None
        _lib.check(_lib.lib().gsvc_msssim_loss_backward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(g), C_, H, W, _lib.ptr(work), _lib.ptr(grads),
                                                        _lib.ptr(d), _lib.ptr(db), _lib.current_stream(a.device)),
                   "gsvc_msssim_loss_backward")
        return d, db, None


def _check_ms_images(name, *imgs):
    if any(t.dim() != 3 or t.shape != imgs[0].shape for t in imgs):
        raise ValueError(f"{name}: images must be [C, H, W] tensors of one shape")


def ms_ssim_l1(img, gt, img_b=None):
    """(metrics.ms_ssim(x, gt, data_range=1), l1_loss_func(x, gt)) of [C,H,W] images, both sides > 160; the gradient goes to ``img``
    (and ``img_b``).  x = img, or with ``img_b`` the two-view frame x = (img + flip(img_b, W)) / 2, then also returned, detached, as a
    third result.  CUDA tensors take the fused kernels of csrc/msssim_loss.hip (eleven launches forward, five backward); CPU tensors
    the tensor expressions, differentiable through autograd."""
    _check_ms_images("ms_ssim_l1", img, gt, *(() if img_b is None else (img_b,)))
    if img.is_cuda:
        return _MsSsimL1.apply(img, img_b, gt)
    from .metrics import ms_ssim
    x = img if img_b is None else (img + torch.flip(img_b, dims=[2])) / 2
    terms = ms_ssim(x, gt, data_range=1), l1_loss_func(x, gt)
    return terms if img_b is None else terms + (x.detach(),)


class _WSsimL1(torch.autograd.Function):
    """``_SsimL1`` with a weight per cell (csrc/wdist.hip): (sum w ssim, sum w |x - gt|) / (C H W)[, x].  The partial maps leave the forward
    kernel multiplied by the weights, so the backward is ``_SsimL1``'s plus the weight in the L1 sign term.  No atomics: the sums are the
    same bits in every run."""

    @staticmethod
    def forward(ctx, img, img_b, gt, weights, cell):
        from . import _lib
        pair = img_b is not None
        a, g, w = img.contiguous().float(), gt.contiguous().float(), weights.contiguous()
        b = img_b.contiguous().float() if pair else None
        C_, H, W = a.shape
        need = img.requires_grad or (pair and img_b.requires_grad)
        L, st = _lib.lib(), _lib.current_stream(a.device)
        sums = torch.empty(2, device=a.device, dtype=torch.float32)
        work = torch.empty(int(L.gsvc_wssim_workspace_floats(C_, H, W)), device=a.device, dtype=torch.float32)
        avg = torch.empty_like(a) if pair else None
        maps = [torch.empty_like(a) for _ in range(3)] if need else [None, None, None]
        _lib.check(L.gsvc_wssim_l1_forward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(g), _lib.ptr(w), C_, H, W, cell, _lib.ptr(sums), _lib.ptr(work),
                                           _lib.ptr(maps[0]), _lib.ptr(maps[1]), _lib.ptr(maps[2]), _lib.ptr(avg), st),
                   "gsvc_wssim_l1_forward")
        if need:
            ctx.save_for_backward(a, g, w, *maps, *((b,) if pair else ()))
        ctx.pair, ctx.cell = pair, cell
        ctx.set_materialize_grads(False)
        out = sums / float(C_ * H * W)
        if pair:
            ctx.mark_non_differentiable(avg)
            return out[0], out[1], avg
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_ssim, g_l1, _g_avg=None):
        from . import _lib
        a, g, w, m0, m1, m2 = ctx.saved_tensors[:6]
        b = ctx.saved_tensors[6] if ctx.pair else None
        C_, H, W = a.shape
        zero = torch.zeros((), device=a.device) if (g_ssim is None or g_l1 is None) else None
        grads = torch.stack([zero if g_ssim is None else g_ssim, zero if g_l1 is None else g_l1]).float().contiguous()
        d = torch.empty_like(a)
        db = torch.empty_like(b) if ctx.pair else None
        _lib.check(_lib.lib().gsvc_wssim_l1_backward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(g), _lib.ptr(w), C_, H, W, ctx.cell, _lib.ptr(grads),
                                                     _lib.ptr(m0), _lib.ptr(m1), _lib.ptr(m2), _lib.ptr(d), _lib.ptr(db),
                                                     _lib.current_stream(a.device)), "gsvc_wssim_l1_backward")
        return d, db, None, None, None


def pixel_weights(weights, cell: int, H: int, W: int):
    """The ``[Hc, Wc]`` cell weights as an ``[H, W]`` picture: pixel (y, x) has ``weights[y // cell][x // cell]``."""
    return weights.repeat_interleave(cell, dim=0).repeat_interleave(cell, dim=1)[:H, :W]


def wssim_l1(img, gt, weights, cell, img_b=None):
    """``ssim_l1`` with a weight per cell of ``cell`` x ``cell`` pixels (4, 8 or 16; ``weights``: float32 ``[ceil(H / cell), ceil(W / cell)]``
    on the images' device, finite and >= 0, gsvc_amd/wdist.py): ``(sum w ssim_map, sum w |x - gt|) / (C H W)`` over the pixels of every
    channel — the weighted means where the map is normalised — and with ``img_b`` the two-view frame x = (img + flip(img_b, W)) / 2 as a
    third, detached result.  The gradient goes to ``img`` (and ``img_b``), none to the weights.  CUDA tensors take the kernels of
    csrc/wdist.hip (no atomics: bit-identical from run to run); CPU tensors the tensor expressions, differentiable through autograd."""
    from .detail import CELLS, map_shape
    _check_ms_images("wssim_l1", img, gt, *(() if img_b is None else (img_b,)))
    if isinstance(cell, bool) or cell not in CELLS:
        raise ValueError(f"wssim_l1: cell must be one of {', '.join(str(c) for c in CELLS)} (got {cell!r})")
    H, W = int(img.shape[1]), int(img.shape[2])
    if tuple(weights.shape) != map_shape(H, W, cell):
        raise ValueError(f"wssim_l1: the weights of a {H} x {W} picture at cell {cell} must be {list(map_shape(H, W, cell))} "
                         f"(got {list(weights.shape)})")
    if img.is_cuda:
        if weights.device != img.device or weights.dtype != torch.float32:
            raise ValueError(f"wssim_l1: the weights must be float32 on {img.device} (got {weights.dtype} on {weights.device})")
        return _WSsimL1.apply(img, img_b, gt, weights, int(cell))
    x = img if img_b is None else (img + torch.flip(img_b, dims=[2])) / 2
    wp = pixel_weights(weights.to(x.dtype), int(cell), H, W)
    terms = (wp * _ssim_map(x.unsqueeze(0), gt.unsqueeze(0))[0]).mean(), (wp * (x - gt).abs()).mean()
    return terms if img_b is None else terms + (x.detach(),)


DISTORTIONS = {"ssim": ssim_l1, "ms_ssim": ms_ssim_l1}      # OptimizationParams.distortion -> the structural term with its L1


class StepDistortion:
    """The distortion of a fitting step: where it is taken (``opt.loss_domain``: float RGB, or the Y'CbCr planes the codec delivers and
    is measured on, gsvc_amd/yuv_loss.py) and its structural term (``opt.distortion``: single-scale SSIM, or MS-SSIM as
    ``metrics.ms_ssim`` reports it), decided once against the dataset a Trainer is built on.  It keeps no dataset: the methods that
    read one take the step's current one.

    ``weight_maps`` (float32 ``[T, Hc, Wc]``, one map per frame of the dataset, at ``weight_cell``: gsvc_amd/wdist.py) weights the image
    terms per cell through ``wssim_l1``; ``__call__`` then needs the frame's index.  Only the rgb domain with the single-scale SSIM
    takes weights."""

    def __init__(self, opt, dataset, weight_maps=None, weight_cell=None):
        if weight_maps is not None:          # said first: what the maps cannot go with, before the dataset is looked at
            if opt.loss_domain != "rgb":
                raise ValueError(f"weight maps are taken on RGB pictures only: loss_domain must be 'rgb' (got {opt.loss_domain!r}); the "
                                 f"weighted plane terms of the yuv domains do not exist")
            if opt.distortion != "ssim":
                raise ValueError(f"weight maps go with distortion 'ssim' only (got {opt.distortion!r}): a weighted MS-SSIM does not exist")
        self.domain = opt.loss_domain
        self.layout = yuv_loss.domain_layout(self.domain)          # of the planes; None in the rgb domain (an unknown name is refused here)
        self.fmt = self.matrix = None
        self.native_planes = False
        if self.layout is not None:
            yuv_loss.check_domain(self.domain, dataset.height, dataset.width)
            yuv_loss.check_dataset(dataset, self.layout)
            self.fmt = yuv_loss.FrameFormat(self.layout, yuv_loss.loss_matrix(dataset))
            self.matrix = self.fmt.matrix
            self.native_planes = yuv_loss.native_planes(dataset, self.layout)      # the targets come from the file's codes: no picture is read
        self.name = opt.distortion
        if self.name not in DISTORTIONS:
            raise ValueError(f"unknown distortion {self.name!r} (one of {', '.join(DISTORTIONS)})")
        if self.name == "ms_ssim":
            if self.domain != "rgb":
                raise ValueError(f"distortion 'ms_ssim' is taken on RGB pictures: loss_domain must be 'rgb' (got {self.domain!r})")
            if min(int(dataset.height), int(dataset.width)) <= 160:
                raise ValueError(f"distortion 'ms_ssim' needs picture sides above 160 pixels for 5 scales "
                                 f"(got {int(dataset.height)} x {int(dataset.width)})")
        self.structural = DISTORTIONS[self.name]
        self.weight_maps = self.weight_cell = None
        if weight_maps is not None:
            from .detail import CELLS, map_shape
            if isinstance(weight_cell, bool) or weight_cell not in CELLS:
                raise ValueError(f"weight_cell must be one of {', '.join(str(c) for c in CELLS)} (got {weight_cell!r})")
            want = (int(dataset.len_z_frames),) + map_shape(int(dataset.height), int(dataset.width), weight_cell)
            if not torch.is_tensor(weight_maps) or tuple(weight_maps.shape) != want:
                got = tuple(weight_maps.shape) if torch.is_tensor(weight_maps) else type(weight_maps).__name__
                raise ValueError(f"weight_maps must be a tensor {list(want)} for this dataset at cell {weight_cell} (got {got})")
            self.weight_maps, self.weight_cell = weight_maps.detach().float().contiguous(), int(weight_cell)

    def frame(self, dataset, i):
        """Frame i of the dataset; without its picture where the step's targets are the file's own planes (a fetch of a
        ``VideoFileCube(resident="u8")`` would launch a conversion nobody reads)."""
        return dataset.get_dummy_frame(i) if self.native_planes else dataset[i]

    def target(self, dataset, frame, i, dev):
        """The ground truth of frame i in the loss domain: the picture [3, H, W], or its planes (tY, tC)."""
        if self.fmt is None:
            return frame.image.to(dev).permute(0, 2, 1).contiguous()
        picture = None if self.native_planes else frame.image.to(dev)
        return yuv_loss.target_planes(dataset, i, self.layout, self.matrix, picture=picture)

    def __call__(self, img_f, img_b, target, frame_index=None):
        """``(terms, image)`` of one frame: its scalar terms, all L1 terms first and then all structural terms — ``(l1, s)`` in rgb,
        ``(l1_y, l1_c, s_y, s_c)`` on planes — and the two-view frame (img_f + flip(img_b, W)) / 2, detached, which the kernels form
        themselves; ``img_b`` None: ``img_f`` is that frame already.  ``frame_index``: the frame's index in the dataset, which picks its
        weight map (needed with ``weight_maps``, unused without)."""
        if self.weight_maps is not None:
            if frame_index is None:
                raise ValueError("StepDistortion: with weight maps the call needs frame_index")
            out = wssim_l1(img_f, target, self.weight_maps[frame_index], self.weight_cell, img_b)
            return (out[1], out[0]), (img_f if img_b is None else out[2]).detach()
        if self.fmt is None:
            out = self.structural(img_f, target, img_b)
            return (out[1], out[0]), (img_f if img_b is None else out[2]).detach()
        terms, avg = yuv_loss.plane_terms(self.structural, img_f, img_b, target, self.fmt)
        return terms, (img_f if img_b is None else avg).detach()

    @staticmethod
    def image_terms(terms1, terms2):
        """The step's image terms of its two frames' tuples, interleaved: ``[l1_1, l1_2, s_1, s_2]`` in rgb.  The loss is
        ``dot(stack(terms), weights)``: the order is that of ``weights`` and decides the sum's bits."""
        return [t for pair in zip(terms1, terms2) for t in pair]

    def weights(self, lambda_dssim):
        """``(weights, const)`` of ``image_terms``: ``yuv_loss.distortion_weights``."""
        return yuv_loss.distortion_weights(self.domain, lambda_dssim)


def l1_loss_func(network_output, gt):
    return (network_output - gt).abs().mean()


def l2_loss_func(network_output, gt):
    return ((network_output - gt) ** 2).mean()


@lru_cache(maxsize=4)
def _window_1d(window_size: int, sigma: float):
    g = torch.tensor([exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)])
    # the taps of make_loss_window() in csrc/ssim_tile.h, bit for bit: the fp32 taps are added one by one in fp32.  (g.sum() adds them in
    # another order; for 11 taps at sigma 1.5 its sum is one ulp larger and nine of the taps come out one ulp smaller.)
    s = g[0]
    for t in g[1:]:
        s = s + t
    return g / s


def _blur(x, w1d, pad):
    """Depthwise separable Gaussian blur of [B,C,H,W] with zero padding."""
    C = x.shape[1]
    kh = w1d.view(1, 1, -1, 1).expand(C, 1, -1, 1)
    kw = w1d.view(1, 1, 1, -1).expand(C, 1, 1, -1)
    x = F.conv2d(x, kh, padding=(pad, 0), groups=C)
    return F.conv2d(x, kw, padding=(0, pad), groups=C)


def ssim_func(img1, img2, window_size=11, size_average=True):
    if img1.is_cuda and window_size == 11:
        # GPU tensors always take the fused HIP kernel (per image when a batch is given)
        if img1.dim() == 3:
            return _SsimL1.apply(img1, None, img2)[0]
        per = torch.stack([_SsimL1.apply(a, None, b)[0] for a, b in zip(img1, img2)])
        return per.mean() if size_average else per
    squeeze = img1.dim() == 3
    a = img1.unsqueeze(0) if squeeze else img1
    b = img2.unsqueeze(0) if squeeze else img2
    ssim_map = _ssim_map(a, b, window_size)
    if size_average:
        return ssim_map.mean()
    return ssim_map.mean(1).mean(1).mean(1)


def _ssim_map(a, b, window_size=11):
    """The SSIM map of two [B,C,H,W] batches as tensor expressions (what ``ssim_func`` averages)."""
    w = _window_1d(window_size, 1.5).to(device=a.device, dtype=a.dtype)
    pad = window_size // 2
    B = a.shape[0]
    m = _blur(torch.cat([a, b, a * a, b * b, a * b], dim=0), w, pad)
    mu1, mu2, e11, e22, e12 = m[:B], m[B:2 * B], m[2 * B:3 * B], m[3 * B:4 * B], m[4 * B:]
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))


def _alive_slots(res, n_offsets):
    """Flat (anchor*K + slot) indices of the Gaussians a render generated (opacity > 0), in generation order."""
    vis = res.visible_mask
    idx = torch.arange(vis.shape[0] * n_offsets, device=vis.device).view(-1, n_offsets)
    return idx[vis].reshape(-1)[res.generated_gaussians.mask]


def _world_xy(res, keep):
    rows = res.generated_gaussians.concatenated_all.index_select(0, keep.nonzero(as_tuple=False).squeeze(1))
    scaling, anchor, offsets = rows[:, 0:6], rows[:, 6:9], rows[:, 19:22]
    return (anchor + offsets * scaling[:, :3])[:, :2]


def calc_optical_loss_one_frame(render_results1, render_results2, optical_flow, x_min, y_min, scale,
                                x_pix_max: int, y_pix_max: int, n_offsets=10):
    """Gaussians alive in both renders (same anchor, same offset slot): their world-xy displacement should
    equal the optical flow sampled at the frame-1 pixel (reference loss_utils.py:76-135)."""
    dev = render_results1.visible_mask.device
    total = render_results1.visible_mask.shape[0] * n_offsets
    alive1 = torch.zeros(total, dtype=torch.bool, device=dev)
    alive2 = torch.zeros(total, dtype=torch.bool, device=dev)
    alive1[_alive_slots(render_results1, n_offsets)] = True
    alive2[_alive_slots(render_results2, n_offsets)] = True
    common = (alive1 & alive2).view(-1, n_offsets)
    keep1 = common[render_results1.visible_mask].reshape(-1) & render_results1.generated_gaussians.mask
    keep2 = common[render_results2.visible_mask].reshape(-1) & render_results2.generated_gaussians.mask
    xy1 = _world_xy(render_results1, keep1)
    xy2 = _world_xy(render_results2, keep2)
    from .generate import host_values
    pix = ((xy1 - host_values([[x_min, y_min]], dev, xy1.dtype)) * scale).round().long()
    ok = (pix[:, 0] >= 0) & (pix[:, 1] >= 0) & (pix[:, 0] < x_pix_max) & (pix[:, 1] < y_pix_max)
    oki = ok.nonzero(as_tuple=False).squeeze(1)
    pix = pix.index_select(0, oki)
    flow = optical_flow.permute(2, 1, 0).to(dev)
    uv = flow[pix[:, 0], pix[:, 1], ...] / scale
    d = xy2.index_select(0, oki) - xy1.index_select(0, oki)
    return (d - uv).abs().mean(), pix, d * scale


class _OpticalPair(torch.autograd.Function):
    """Optical-flow consistency of one adjacent-frame pair over un-compacted renders (csrc/losses.hip)."""

    @staticmethod
    def forward(ctx, world1, world2, mask1, mask2, vis1, vis2, flow, K, anchors, x_min, y_min, scale, x_pix_max, y_pix_max):
        from . import _lib
        dev = world1.device
        world1, world2 = world1.contiguous(), world2.contiguous()
        m1, m2 = mask1.contiguous().view(torch.uint8), mask2.contiguous().view(torch.uint8)
        flow = flow.contiguous()
        n1, n2 = world1.shape[0], world2.shape[0]
        table = torch.empty(anchors * K, dtype=torch.int32, device=dev)
        partner = torch.empty(max(n1, 1), dtype=torch.int32, device=dev)
        sums = torch.empty(2, dtype=torch.float32, device=dev)
        partial = torch.empty(2 * max((n1 + 255) // 256, 1), dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().gsvc_optical_forward(
            _lib.ptr(world1), _lib.ptr(m1), _lib.ptr(vis1.contiguous()), n1, _lib.ptr(world2), _lib.ptr(m2), _lib.ptr(vis2.contiguous()),
            n2, K, anchors, _lib.ptr(flow), flow.shape[1], flow.shape[2], float(x_min), float(y_min), float(scale), int(x_pix_max),
            int(y_pix_max), _lib.ptr(table), _lib.ptr(partner), _lib.ptr(sums), _lib.ptr(partial), _lib.current_stream(dev)),
            "gsvc_optical_forward")
        ctx.save_for_backward(partner, sums)
        ctx.n = (n1, n2)
        return sums[0] / (2.0 * sums[1])

    @staticmethod
    def backward(ctx, g):
        from . import _lib
        partner, sums = ctx.saved_tensors
        n1, n2 = ctx.n
        dev = partner.device
        g1 = torch.empty(n1, 3, dtype=torch.float32, device=dev)
        g2 = torch.empty(n2, 3, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().gsvc_optical_backward(_lib.ptr(partner), n1, n2, _lib.ptr(sums), _lib.ptr(g.contiguous().float()),
                                                    _lib.ptr(g1), _lib.ptr(g2), _lib.current_stream(dev)), "gsvc_optical_backward")
        return (g1, g2) + (None,) * 12


def _optical_loss_dense(r1, r2, optical_flow, x_min, y_min, scale, x_pix_max: int, y_pix_max: int, n_offsets=10):
    """calc_optical_loss_one_frame for un-compacted results (render_many(dense=True)): the "alive in both renders"
    intersection and the pairing of the two renders' Gaussians go through an [anchors*K] slot table inside the fused
    kernels of csrc/losses.hip — the same mean over the same pairs, with no compaction and no host synchronisation."""
    g1, g2 = r1.generated_gaussians, r2.generated_gaussians
    return _OpticalPair.apply(g1.world_xyz, g2.world_xyz, g1.mask, g2.mask, r1.visible_index, r2.visible_index,
                              optical_flow.to(g1.world_xyz.device), n_offsets, r1.visible_mask.shape[0], x_min, y_min, scale,
                              x_pix_max, y_pix_max)


class _OpticalMany(torch.autograd.Function):
    """calc_optical_loss over renders that are row ranges of one set of tensors (render_many(dense=True)): every pair in four
    launches forward and one backward, the gradient in the concatenated layout (csrc/losses.hip k_optical_*_many)."""

    @staticmethod
    def forward(ctx, world, mask, vis, goff, pairs, flow, K, anchors, x_min, y_min, scale, x_pix_max, y_pix_max):
        import ctypes as C
        from . import _lib
        dev = world.device
        world, vis, flow = world.contiguous(), vis.contiguous(), flow.contiguous()
        m = mask.contiguous().view(torch.uint8)
        R, P = len(goff) - 1, len(pairs)
        off = (C.c_int64 * (R + 1))(*[int(v) for v in goff])
        src, dst = (C.c_int32 * P)(*[p[0] for p in pairs]), (C.c_int32 * P)(*[p[1] for p in pairs])
        L = _lib.lib()
        table = torch.empty(R * anchors, dtype=torch.int32, device=dev)
        partner = torch.empty(max(int(goff[-1]), 1), dtype=torch.int32, device=dev)
        res = torch.empty(2 * P + 1 + int(L.gsvc_optical_many_partial_floats(off, R, src, dst, P, K)), dtype=torch.float32, device=dev)
        sums, loss, partial = res[:2 * P], res[2 * P:2 * P + 1], res[2 * P + 1:]
        _lib.check(L.gsvc_optical_many_forward(_lib.ptr(world), _lib.ptr(m), _lib.ptr(vis), off, R, src, dst, P, K, anchors, _lib.ptr(flow),
                                               flow.shape[1], flow.shape[2], float(x_min), float(y_min), float(scale), int(x_pix_max),
                                               int(y_pix_max), _lib.ptr(table), _lib.ptr(partner), _lib.ptr(sums), C.c_void_p(partial.data_ptr()),
                                               C.c_void_p(loss.data_ptr()), _lib.current_stream(dev)), "gsvc_optical_many_forward")
        ctx.save_for_backward(partner, vis, table, sums)
        ctx.meta = (off, R, src, dst, P, K, anchors, world.shape)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        from . import _lib
        partner, vis, table, sums = ctx.saved_tensors
        off, R, src, dst, P, K, anchors, shape = ctx.meta
        gw = torch.empty(shape, dtype=torch.float32, device=partner.device)
        _lib.check(_lib.lib().gsvc_optical_many_backward(_lib.ptr(partner), _lib.ptr(vis), off, R, src, dst, P, K, anchors, _lib.ptr(table),
                                                         _lib.ptr(sums), _lib.ptr(g.contiguous().float()), _lib.ptr(gw),
                                                         _lib.current_stream(partner.device)), "gsvc_optical_many_backward")
        return (gw,) + (None,) * 12


class _RenderRegs(torch.autograd.Function):
    """(sum_r mean over opacity>0 of prod(scaling), sum_r mean(1 - neural_opacity)) over the concatenated
    un-compacted Gaussians of R renders (csrc/losses.hip)."""

    @staticmethod
    def forward(ctx, scaling, neural_opacity, mask, seg_offsets):
        import ctypes as C
        from . import _lib
        dev = scaling.device
        scaling, op = scaling.contiguous(), neural_opacity.contiguous()
        m = mask.contiguous().view(torch.uint8)
        R = len(seg_offsets) - 1
        seg = (C.c_int64 * (R + 1))(*[int(v) for v in seg_offsets])
        L = _lib.lib()
        sums = torch.empty(3 * R, dtype=torch.float32, device=dev)
        partial = torch.empty(int(L.gsvc_regs_partial_floats(seg, R)), dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.check(L.gsvc_regs_forward(_lib.ptr(scaling), _lib.ptr(op), _lib.ptr(m), seg, R, _lib.ptr(sums), _lib.ptr(partial),
                                       _lib.ptr(out), _lib.current_stream(dev)), "gsvc_regs_forward")
        ctx.save_for_backward(scaling, m, sums)
        ctx.seg, ctx.R, ctx.op_shape = seg, R, neural_opacity.shape
        ctx.set_materialize_grads(False)
        return out[0], out[1]      # two scalars (indexing a returned 2-vector costs a zero-fill + copy + add per element in the backward)

    @staticmethod
    def backward(ctx, g0, g1):
        from . import _lib
        scaling, m, sums = ctx.saved_tensors
        dev = scaling.device
        if g0 is None and g1 is None:
            return None, None, None, None
        zero = torch.zeros((), device=dev) if (g0 is None or g1 is None) else None
        g = torch.stack([zero if g0 is None else g0, zero if g1 is None else g1])
        gs = torch.empty_like(scaling)
        go = torch.empty(scaling.shape[0], dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().gsvc_regs_backward(_lib.ptr(scaling), _lib.ptr(m), ctx.seg, ctx.R, _lib.ptr(sums),
                                                 _lib.ptr(g.contiguous().float()), _lib.ptr(gs), _lib.ptr(go),
                                                 _lib.current_stream(dev)), "gsvc_regs_backward")
        return gs, go.view(ctx.op_shape), None, None


def render_regs(scaling, neural_opacity, mask, seg_offsets):
    """Returns the pair (scaling regulariser, opacity regulariser) summed over the renders delimited by seg_offsets."""
    return _RenderRegs.apply(scaling, neural_opacity, mask, seg_offsets)


def calc_optical_loss(render_results1_f, render_results1_b, render_results2_f, render_results2_b, optical_flow,
                      x_min, y_min, scale, x_pix_max: int, y_pix_max: int, n_offsets=10):
    if render_results1_f.dense:
        rs = (render_results1_f, render_results1_b, render_results2_f, render_results2_b)
        # (getattr: callers hand this function renders of their own making, whose Gaussians are any object with world_xyz / mask)
        batch = getattr(rs[0].generated_gaussians, "batch", None)
        if (batch is not None and batch.world.is_cuda and len(batch.seg_offsets) == 5
                and all(r.generated_gaussians.batch is batch for r in rs)):
            # the four renders are row ranges of the batch's tensors, in this order: both pairs in one pass
            return _OpticalMany.apply(batch.world, batch.mask, batch.vis, batch.seg_offsets, ((0, 2), (1, 3)),
                                      optical_flow.to(batch.world.device), n_offsets, rs[0].visible_mask.shape[0], x_min, y_min, scale,
                                      x_pix_max, y_pix_max)
        args = (optical_flow, x_min, y_min, scale, x_pix_max, y_pix_max, n_offsets)
        return (_optical_loss_dense(render_results1_f, render_results2_f, *args)
                + _optical_loss_dense(render_results1_b, render_results2_b, *args))
    lf, _, _ = calc_optical_loss_one_frame(render_results1_f, render_results2_f, optical_flow, x_min, y_min, scale,
                                           x_pix_max, y_pix_max, n_offsets)
    lb, _, _ = calc_optical_loss_one_frame(render_results1_b, render_results2_b, optical_flow, x_min, y_min, scale,
                                           x_pix_max, y_pix_max, n_offsets)
    return lf + lb


def psnr_func(img1, img2, data_range=1):
    """reference utils/metric_utils.py:10-13"""
    return 10 * torch.log10((data_range ** 2) / torch.mean((img1 - img2) ** 2))
