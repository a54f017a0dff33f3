"""The fitting step's distortion in the delivered domain: L1 + SSIM on float Y'CbCr planes (host side of csrc/yuv_loss.hip).

The codec reads Y'CbCr files (``frames_in.VideoFileCube``) and is measured on Y'CbCr sample codes (``metrics.code_metrics``); with
``OptimizationParams.loss_domain = "yuv420"`` or ``"yuv444"`` the step fits there too.  A picture becomes a plane buffer
``[Y: H W | Cb: ch cw | Cr: ch cw]`` of float32 (include/gsvc_hip.h), seen as ``Y [1, H, W]`` and ``C [2, ch, cw]``; luma is the Y of
``frames_out``'s formulas and chroma its ``C + 0.5``, nothing clamped.  ``yuv_planes`` makes the planes of a render (differentiable:
one HIP kernel each way), ``frame_planes`` those of a file's sample codes with no chroma upsampling, and ``yuv_ssim_l1`` runs the
SSIM / L1 kernels of ``loss_utils`` on luma (C = 1) and on the chroma pair (C = 2).

Importing this module needs neither a GPU nor the built library; every function that computes needs both (no CPU fallback).
"""
from __future__ import annotations

import torch

from .frames_out import LAYOUTS, MATRICES, MAX_BATCH, RANGES, FrameFormat, frame_bytes

DOMAINS = {"rgb": None, "yuv420": "yuv420p", "yuv444": "yuv444p"}      # OptimizationParams.loss_domain -> the layout of the planes
LUMA_WEIGHT, CHROMA_WEIGHT = 0.75, 0.25                                # 6 : 1 : 1 over Y, Cb, Cr (the weighting of metrics.code_metrics)


def domain_layout(domain: str):
    """The plane layout of a loss domain (None for ``"rgb"``); anything else than the three names is refused."""
    if domain not in DOMAINS:
        raise ValueError(f"unknown loss_domain {domain!r} (one of {', '.join(DOMAINS)})")
    return DOMAINS[domain]


def check_domain(domain: str, H: int, W: int):
    """``domain_layout`` plus the size rule of 4:2:0."""
    layout = domain_layout(domain)
    if layout == "yuv420p" and (int(H) % 2 or int(W) % 2):
        raise ValueError(f"loss_domain 'yuv420' needs even H and W (got {int(H)} x {int(W)})")
    return layout


def distortion_weights(domain: str, lambda_dssim: float):
    """``(weights, const)`` of the image terms of a step's two frames: the loss takes ``dot(terms, weights) + const``.  The terms are
    the two frames' tuples of ``loss_utils.StepDistortion`` — a frame's L1 terms, then its structural terms — interleaved.

    ``"rgb"``: terms ``[l1_1, l1_2, ssim_1, ssim_2]``, D = (1 - l) L1 + l (1 - SSIM) per frame.  A yuv domain: terms ``[l1_y1, l1_y2,
    l1_c1, l1_c2, ssim_y1, ssim_y2, ssim_c1, ssim_c2]`` and D = 0.75 D_Y + 0.25 D_C per frame, D_C over both chroma planes: the 6:1:1
    weighting on the scale of the RGB distortion, so that ``lmbda`` keeps its meaning to first order."""
    lam = float(lambda_dssim)
    if domain_layout(domain) is None:
        return [1.0 - lam] * 2 + [-lam] * 2, 2.0 * lam
    w = (LUMA_WEIGHT, LUMA_WEIGHT, CHROMA_WEIGHT, CHROMA_WEIGHT)
    return [(1.0 - lam) * v for v in w] + [-lam * v for v in w], 2.0 * lam * (LUMA_WEIGHT + CHROMA_WEIGHT)


def plane_shapes(H: int, W: int, layout: str):
    """``((1, H, W), (2, ch, cw))`` of a picture's planes."""
    H, W = int(H), int(W)
    if layout == "yuv444p":
        return (1, H, W), (2, H, W)
    if layout != "yuv420p":
        raise ValueError(f"a picture has planes in the layouts yuv420p and yuv444p, not {layout!r}")
    if H % 2 or W % 2:
        raise ValueError(f"yuv420p needs even H and W (got {H} x {W})")
    return (1, H, W), (2, H // 2, W // 2)


def split_planes(planes, H: int, W: int, layout: str):
    """Views ``(Y [1, H, W], C [2, ch, cw])`` of one flat plane buffer."""
    ys, cs = plane_shapes(H, W, layout)
    n = ys[1] * ys[2]
    return planes[:n].view(ys), planes[n:n + 2 * cs[1] * cs[2]].view(cs)


class _YuvPlanes(torch.autograd.Function):
    """(Y, C, a) of a = (img_f + flip_W(img_b)) / 2 (a = img_f without img_b): csrc/yuv_loss.hip, one kernel each way."""

    @staticmethod
    def forward(ctx, img_f, img_b, layout, matrix):
        from . import _lib
        f = img_f.contiguous().float()
        b = img_b.contiguous().float() if img_b is not None else None
        _, H, W = f.shape
        ys, cs = plane_shapes(H, W, layout)
        planes = torch.empty(H * W + 2 * cs[1] * cs[2], device=f.device, dtype=torch.float32)
        avg = torch.empty_like(f)
        _lib.check(_lib.lib().gsvc_yuv_planes_forward(_lib.ptr(f), _lib.ptr(b), H, W, LAYOUTS[layout], MATRICES[matrix], _lib.ptr(planes),
                                                      _lib.ptr(avg), _lib.current_stream(f.device)), "gsvc_yuv_planes_forward")
        ctx.meta = (H, W, layout, matrix, b is not None)
        ctx.mark_non_differentiable(avg)
        ctx.set_materialize_grads(False)      # no zero image for the averaged frame's (absent) gradient
        Y, C = split_planes(planes, H, W, layout)
        return Y, C, avg

    @staticmethod
    def backward(ctx, g_y, g_c, _g_avg):
        from . import _lib
        H, W, layout, matrix, pair = ctx.meta
        if g_y is None and g_c is None:
            return None, None, None, None
        ys, cs = plane_shapes(H, W, layout)
        dev = (g_y if g_y is not None else g_c).device
        # the SSIM backward of either term writes a tensor of its own: one launch joins them into the plane-buffer layout
        d_planes = torch.cat([(g_y if g_y is not None else torch.zeros(ys, device=dev)).reshape(-1).float(),
                              (g_c if g_c is not None else torch.zeros(cs, device=dev)).reshape(-1).float()])
        df = torch.empty((3, H, W), device=dev, dtype=torch.float32)
        db = torch.empty_like(df) if pair else None
        _lib.check(_lib.lib().gsvc_yuv_planes_backward(_lib.ptr(d_planes), H, W, LAYOUTS[layout], MATRICES[matrix], _lib.ptr(df),
                                                       _lib.ptr(db), _lib.current_stream(dev)), "gsvc_yuv_planes_backward")
        return df, db, None, None


def _check_names(layout: str, matrix: str):
    if layout not in ("yuv420p", "yuv444p"):
        raise ValueError(f"a picture has planes in the layouts yuv420p and yuv444p, not {layout!r}")
    if matrix not in MATRICES:
        raise ValueError(f"unknown matrix {matrix!r} (one of {', '.join(MATRICES)})")


def yuv_planes(img_f, img_b=None, layout: str = "yuv420p", matrix: str = "bt709"):
    """``(Y [1, H, W], C [2, ch, cw], a)`` of the two-view frame a = (img_f + flip(img_b, W)) / 2 — a = img_f when ``img_b`` is None —
    for ``[3, H, W]`` CUDA images.  Differentiable with respect to both images; ``a`` is not."""
    _check_names(layout, matrix)
    if not img_f.is_cuda:
        from . import _lib
        raise _lib.GsvcError("yuv_planes runs on the HIP kernels of csrc/yuv_loss.hip; CPU tensors are not supported")
    if img_f.dim() != 3 or img_f.shape[0] != 3 or (img_b is not None and img_b.shape != img_f.shape):
        raise ValueError(f"yuv_planes: images must be [3, H, W] of one size (got {tuple(img_f.shape)}"
                         f"{'' if img_b is None else ' and ' + str(tuple(img_b.shape))})")
    plane_shapes(img_f.shape[1], img_f.shape[2], layout)
    return _YuvPlanes.apply(img_f, img_b, layout, matrix)


def plane_terms(structural, img_f, img_b, target, fmt: FrameFormat):
    """``((l1_y, l1_c, s_y, s_c), a)``: ``structural(x, gt) -> (s, l1)`` (``loss_utils.ssim_l1``) taken of the luma plane (C = 1) and
    of the two chroma planes (C = 2) of the two-view frame against ``target = (tY, tC)`` (``target_planes``, ``frame_planes`` +
    ``split_planes``) in the layout and matrix of ``fmt``; autograd chains the terms' backward into the transform's."""
    tY, tC = target
    Y, C, avg = yuv_planes(img_f, img_b, fmt.layout, fmt.matrix)
    s_y, l1_y = structural(Y, tY)
    s_c, l1_c = structural(C, tC)
    return (l1_y, l1_c, s_y, s_c), avg


def yuv_ssim_l1(img_f, img_b, target, fmt: FrameFormat):
    """``(ssim_y, l1_y, ssim_c, l1_c, a)``: ``plane_terms`` with mean SSIM (the kernels of ``loss_utils.ssim_l1``) as the structural
    term."""
    from .loss_utils import ssim_l1
    (l1_y, l1_c, ssim_y, ssim_c), avg = plane_terms(ssim_l1, img_f, img_b, target, fmt)
    return ssim_y, l1_y, ssim_c, l1_c, avg


def frame_planes(frames_u8, H: int, W: int, fmt: FrameFormat = FrameFormat(), out=None):
    """uint8 CUDA frames ``[n, >= frame_bytes]`` with contiguous rows (or one flat frame) of a planar Y'CbCr format -> float32
    ``[n, H W + 2 ch cw]`` plane buffers on their device, one launch per 16 frames on the current stream; nothing synchronises.  As in
    ``frames_from_u8`` the buffer holds bytes: a deep format reads little-endian 16-bit samples from it.  There is no matrix and no
    chroma upsampling in this direction: a sample code becomes one float."""
    import ctypes as C

    from . import _lib
    if not isinstance(frames_u8, torch.Tensor):
        raise ValueError(f"frame_planes: frames must be a uint8 tensor (got {type(frames_u8).__name__})")
    if not frames_u8.is_cuda:
        raise _lib.GsvcError("frame_planes runs on the HIP kernels of csrc/yuv_loss.hip; CPU tensors are not supported")
    if fmt.layout not in ("yuv420p", "yuv444p"):
        raise ValueError(f"frame_planes: {fmt.layout} frames hold no Y'CbCr planes")
    H, W = int(H), int(W)
    nbytes = frame_bytes(H, W, fmt)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() not in (1, 2):
        raise ValueError(f"frame_planes: frames must be uint8 [n, >= {nbytes}] or one flat frame (got {frames_u8.dtype} "
                         f"{tuple(frames_u8.shape)})")
    if frames_u8.dim() == 1:
        frames_u8 = frames_u8.unsqueeze(0)
    n = int(frames_u8.shape[0])
    if n < 1 or frames_u8.shape[1] < nbytes or frames_u8.stride(1) != 1 or (n > 1 and frames_u8.stride(0) < nbytes):
        raise ValueError(f"frame_planes: a {fmt.name} frame of {H} x {W} has {nbytes} bytes; frames must be [n >= 1, >= {nbytes}] "
                         f"with contiguous rows (got {tuple(frames_u8.shape)}, strides {tuple(frames_u8.stride())})")
    floats = nbytes // (2 if fmt.depth > 8 else 1)
    dev = frames_u8.device
    if out is None:
        out = torch.empty((n, floats), dtype=torch.float32, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (n, floats)
          or not out[0].is_contiguous()):
        raise ValueError(f"frame_planes: out must be float32 [{n}, {floats}] on {dev} with contiguous rows")
    L = _lib.lib()
    stride = int(frames_u8.stride(0)) if n > 1 else max(int(frames_u8.stride(0)), nbytes)
    if fmt.depth > 8 and n == 1:
        stride += stride & 1          # (one frame: the stride addresses nothing)
    base, obase, ostride = frames_u8.data_ptr(), out.data_ptr(), int(out.stride(0)) * 4
    with torch.cuda.device(dev):
        stream = _lib.current_stream(dev)
        for i in range(0, n, MAX_BATCH):
            m = min(MAX_BATCH, n - i)
            ptrs = (C.c_void_p * m)(*[obase + (i + k) * ostride for k in range(m)])
            _lib.check(L.gsvc_frames_planes(base + i * stride, stride, m, H, W, LAYOUTS[fmt.layout], RANGES[fmt.range], fmt.depth, ptrs,
                                            stream), "gsvc_frames_planes")
    return out


def native_planes(dataset, layout: str) -> bool:
    """Whether ``dataset`` hands out plane buffers of ``layout`` itself (a Y'CbCr video file of that layout: ``VideoFileCube``, also
    behind an ``EstimatedFlowCube``)."""
    fmt = getattr(dataset, "fmt", None)
    return getattr(dataset, "yuv_planes", None) is not None and getattr(fmt, "layout", None) == layout


def loss_matrix(dataset) -> str:
    """The matrix of a dataset that has a Y'CbCr format, else BT.709."""
    fmt = getattr(dataset, "fmt", None)
    return fmt.matrix if getattr(fmt, "layout", None) in ("yuv420p", "yuv444p") else "bt709"


def check_dataset(dataset, layout: str):
    """A 4:2:0 file cannot be fitted in the 4:4:4 domain: three quarters of the chroma it would be compared against do not exist."""
    fmt = getattr(dataset, "fmt", None)
    if layout == "yuv444p" and getattr(fmt, "layout", None) == "yuv420p":
        raise ValueError("loss_domain 'yuv444' on a yuv420p file: the file has no chroma at full resolution to compare against "
                         "(use 'yuv420')")


def target_planes(dataset, i: int, layout: str, matrix: str, picture=None):
    """The ground-truth planes ``(tY [1, H, W], tC [2, ch, cw])`` of frame ``i``: the dataset's own ``yuv_planes(i)`` where it has one
    in the requested layout (the file's sample codes, no invented chroma), else the transform of its RGB picture (synthetic cubes,
    PNG cubes, ``rgb24`` files, and a 4:4:4 file fitted in the 4:2:0 domain).  ``picture``: that RGB picture ``[3, W, H]`` (the cubes
    keep their pictures transposed) when the caller has fetched it already; it is then not fetched again."""
    _check_names(layout, matrix)
    check_dataset(dataset, layout)
    H, W = int(dataset.height), int(dataset.width)
    if native_planes(dataset, layout):
        return split_planes(dataset.yuv_planes(i), H, W, layout)
    if picture is None:
        picture = dataset[i].image
        ready = getattr(dataset, "ready", None)
        if ready is not None:
            ready(i)
    with torch.no_grad():
        Y, C, _ = yuv_planes(picture.permute(0, 2, 1).contiguous(), None, layout, matrix)
    return Y, C
