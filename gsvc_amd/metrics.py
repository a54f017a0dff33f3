"""Evaluation metrics of the reference's report loop on the device: PSNR and MS-SSIM.

``psnr_func`` and ``msssim_fn`` keep the names and argument meaning of reference utils/metric_utils.py:11-37.  The
reference takes MS-SSIM from the third-party package ``pytorch_msssim`` (not in its tree, version not pinned); this is a
restatement of that package's published algorithm (Wang et al. 2003 as implemented there: 11-tap Gaussian window with
sigma 1.5 applied separably WITHOUT padding, 5 scales halved by 2x2 average pooling, contrast-structure terms of the
first four scales and the full SSIM of the last, exponents 0.0448 / 0.2856 / 0.3001 / 0.2363 / 0.1333, negative terms
clipped to 0) — parity unpinned, checked against an independent NumPy / SciPy implementation in tests/test_golden_host.py.
LPIPS: gsvc_amd/lpips.py (needs a weights file).  Plain torch ops: these run a few times per evaluation, not per step.

The metrics a video codec is judged by run as kernels (csrc/metrics.hip; formulas in include/gsvc_hip.h): ``plane_sse`` and
``code_metrics`` take PSNR-Y / -U / -V on the sample CODES of two frame buffers, ``ms_ssim_fused`` is ``ms_ssim`` in ten launches,
``compare_videos`` compares two video files, ``picture_hash`` (csrc/picture_hash.hip) is the per-plane hash a bitstream file carries and
``plane_histograms`` (csrc/scene.hip) the per-plane code histogram the scene-cut detector reads.  These need the built library and a GPU
(no CPU fallback); importing this module does not.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib
from .loss_utils import psnr_func  # noqa: F401  (re-export: reference utils/metric_utils.py:11-14)

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def _gauss_window(size: int, sigma: float, device, dtype):
    x = torch.arange(size, dtype=dtype, device=device) - size // 2
    g = torch.exp(-(x ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def _filter(x, win):
    """Separable valid (unpadded) convolution of every channel with the 1-D window along H, then W."""
    c = x.shape[1]
    k = win.numel()
    if x.shape[2] >= k:
        x = F.conv2d(x, win.view(1, 1, k, 1).expand(c, 1, k, 1), groups=c)
    if x.shape[3] >= k:
        x = F.conv2d(x, win.view(1, 1, 1, k).expand(c, 1, 1, k), groups=c)
    return x


def _ssim_cs(x, y, win, data_range, K=(0.01, 0.03)):
    c1, c2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    mu1, mu2 = _filter(x, win), _filter(y, win)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1 = _filter(x * x, win) - mu1_sq
    s2 = _filter(y * y, win) - mu2_sq
    s12 = _filter(x * y, win) - mu12
    cs_map = (2 * s12 + c2) / (s1 + s2 + c2)
    ssim_map = ((2 * mu12 + c1) / (mu1_sq + mu2_sq + c1)) * cs_map
    return ssim_map.flatten(2).mean(-1), cs_map.flatten(2).mean(-1)


def ms_ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, size_average: bool = True, win_size: int = 11,
            win_sigma: float = 1.5, weights=MS_WEIGHTS) -> torch.Tensor:
    """Multi-scale SSIM of two image batches [N, C, H, W] (a [C, H, W] image is taken as a batch of one)."""
    if x.dim() == 3:
        x, y = x.unsqueeze(0), y.unsqueeze(0)
    if x.shape != y.shape or x.dim() != 4:
        raise ValueError("ms_ssim: inputs must be two [N, C, H, W] tensors of the same shape")
    levels = len(weights)
    if min(x.shape[-2:]) <= (win_size - 1) * 2 ** (levels - 1):
        raise ValueError(f"ms_ssim: image sides must exceed {(win_size - 1) * 2 ** (levels - 1)} pixels for {levels} scales")
    x, y = x.float(), y.float()
    win = _gauss_window(win_size, win_sigma, x.device, x.dtype)
    mcs = []
    for i in range(levels):
        ssim_c, cs = _ssim_cs(x, y, win, data_range)
        if i < levels - 1:
            mcs.append(torch.relu(cs))
            pad = [s % 2 for s in x.shape[2:]]
            x = F.avg_pool2d(x, kernel_size=2, padding=pad)
            y = F.avg_pool2d(y, kernel_size=2, padding=pad)
    terms = torch.stack(mcs + [torch.relu(ssim_c)], dim=0)                      # [levels, N, C]
    w = torch.tensor(weights, dtype=x.dtype, device=x.device).view(-1, 1, 1)
    val = torch.prod(terms ** w, dim=0)
    return val.mean() if size_average else val.mean(1)


def msssim_fn(output, target):
    """reference utils/metric_utils.py:33-37"""
    assert output.size(-2) >= 160
    return ms_ssim(output.float().detach(), target.detach(), data_range=1, size_average=True)


# ----------------------------------------------------------------------------------------------------------------------------
# kernels (csrc/metrics.hip)
# ----------------------------------------------------------------------------------------------------------------------------
SAMPLE_F32, SAMPLE_U8, SAMPLE_U16 = 0, 1, 2                            # the GSVC_SAMPLE_* enums of include/gsvc_hip.h
_MS_MIN_SIDE = 160                                                     # a side must EXCEED this (the rule of ms_ssim)


def _frame_rows(t, nbytes: int, fmt, what: str):
    """uint8 CUDA ``[n, >= nbytes]`` with contiguous rows (or one flat frame) -> (the 2-D tensor, n, stride in bytes)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: frames must be a uint8 tensor (got {type(t).__name__})")
    if not t.is_cuda:
        raise _lib.GsvcError(f"{what} runs on the HIP kernels of csrc/metrics.hip; CPU tensors are not supported")
    if t.dtype != torch.uint8 or t.dim() not in (1, 2):
        raise ValueError(f"{what}: frames must be uint8 [n, >= {nbytes}] or one flat frame (got {t.dtype} {tuple(t.shape)})")
    if t.dim() == 1:
        t = t.unsqueeze(0)
    n = int(t.shape[0])
    if n < 1 or t.shape[1] < nbytes or t.stride(1) != 1 or (n > 1 and t.stride(0) < nbytes):
        raise ValueError(f"{what}: a {fmt.name} frame has {nbytes} bytes; frames must be [n >= 1, >= {nbytes}] with contiguous rows "
                         f"(got {tuple(t.shape)}, strides {tuple(t.stride())})")
    stride = int(t.stride(0)) if n > 1 else max(int(t.stride(0)), nbytes)
    if fmt.depth > 8 and n == 1:
        stride += stride & 1          # (one frame: the stride addresses nothing)
    return t, n, stride


def plane_sse(a_u8, b_u8, H: int, W: int, fmt) -> torch.Tensor:
    """Sum of squared code differences per frame and plane of two frame buffers: uint8 CUDA ``[n, >= frame_bytes]`` with contiguous
    rows (deep formats: little-endian 16-bit samples, even base and row stride) -> int64 ``[n, 3]`` (Y, U, V; R, G, B for ``rgb24``),
    exact.  One launch on the current stream; nothing synchronises."""
    from .frames_out import LAYOUTS, frame_bytes
    H, W = int(H), int(W)
    nbytes = frame_bytes(H, W, fmt)
    a, n, sa = _frame_rows(a_u8, nbytes, fmt, "plane_sse")
    b, nb, sb = _frame_rows(b_u8, nbytes, fmt, "plane_sse")
    if nb != n or a.device != b.device:
        raise ValueError(f"plane_sse: the two buffers must hold the same number of frames on one device (got {n} and {nb})")
    out = torch.empty((n, 3), dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().gsvc_frames_sse(a.data_ptr(), sa, b.data_ptr(), sb, n, H, W, LAYOUTS[fmt.layout], fmt.depth, out.data_ptr(),
                                              _lib.current_stream(a.device)), "gsvc_frames_sse")
    return out


def picture_hash(frames_u8, H: int, W: int, fmt) -> torch.Tensor:
    """The picture hash of every frame and plane of a buffer of delivered frames (what ``plane_sse`` accepts) -> int64 ``[n, 3]`` on
    their device: the bits of the uint64 sums ``gsvc_picture_hash`` defines (include/gsvc_hip.h; the ``PHSH`` section of a bitstream
    file, gsvc_amd/bitstream.py).  One launch on the current stream; nothing synchronises."""
    from .frames_out import LAYOUTS, frame_bytes
    H, W = int(H), int(W)
    nbytes = frame_bytes(H, W, fmt)
    a, n, sa = _frame_rows(frames_u8, nbytes, fmt, "picture_hash")
    out = torch.empty((n, 3), dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().gsvc_picture_hash(a.data_ptr(), sa, n, H, W, LAYOUTS[fmt.layout], fmt.depth, out.data_ptr(),
                                                _lib.current_stream(a.device)), "gsvc_picture_hash")
    return out


def plane_histograms(frames_u8, H: int, W: int, fmt) -> torch.Tensor:
    """The code histogram of every frame and plane of a buffer of delivered frames (what ``picture_hash`` accepts) -> int32
    ``[n, 3, 256]`` on their device: ``out[f, p, b]`` counts the samples of plane ``p`` (``rgb24``: channel ``p``) of frame ``f`` with
    ``min(code >> (depth - 8), 255) == b`` (include/gsvc_hip.h, gsvc_frames_histogram; csrc/scene.hip).  What ``scene.histogram_distance``
    reads.  One launch and the memset on the current stream; nothing synchronises."""
    from .frames_out import LAYOUTS, frame_bytes
    H, W = int(H), int(W)
    nbytes = frame_bytes(H, W, fmt)
    a, n, sa = _frame_rows(frames_u8, nbytes, fmt, "plane_histograms")
    out = torch.empty((n, 3, 256), dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().gsvc_frames_histogram(a.data_ptr(), sa, n, H, W, LAYOUTS[fmt.layout], fmt.depth, out.data_ptr(),
                                                    _lib.current_stream(a.device)), "gsvc_frames_histogram")
    return out


def _msssim_terms(x, y, P: int, H: int, W: int, x_pitch, y_pitch, sample_type: int, peak: float) -> torch.Tensor:
    """gsvc_msssim on P planes starting at the first element of two tensors (pitches = (row, plane) in samples of ``sample_type``; a
    buffer of bytes may hold 16-bit samples): float64 ``[5, P]`` on their device."""
    L = _lib.lib()
    need = int(L.gsvc_msssim_workspace_bytes(P, H, W))
    if need < 0:
        raise ValueError(f"ms_ssim_fused: image sides must exceed {_MS_MIN_SIDE} pixels for 5 scales and P be 1 .. 65535 "
                         f"(got {P} planes of {H} x {W})")
    ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    out = torch.empty((5, P), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.gsvc_msssim(x.data_ptr(), x_pitch[0], x_pitch[1], y.data_ptr(), y_pitch[0], y_pitch[1], P, H, W,
                                 sample_type, float(peak), ws.data_ptr(), out.data_ptr(), _lib.current_stream(x.device)),
                   "gsvc_msssim")
    return out


def _msssim_value(terms: torch.Tensor) -> torch.Tensor:
    """float64 ``[5, ...]`` means -> the product of relu(term) ** weight over the scales, in float64.  The five factors are multiplied
    one after the other: the value of a plane does not depend on how many planes the call holds (a reduction's order may)."""
    val = None
    for k, w in enumerate(MS_WEIGHTS):
        f = torch.relu(terms[k]) ** w
        val = f if val is None else val * f
    return val


def ms_ssim_fused(x: torch.Tensor, y: torch.Tensor, size_average: bool = True, terms: bool = False):
    """``ms_ssim(x, y, data_range=1)`` of CUDA float32 ``[N, C, H, W]`` (or ``[C, H, W]``) through the fused kernels: two launches per
    scale and one that adds up, nothing synchronises.  The per-scale means are float64 and so is the result (``size_average``: one
    number, else ``[N]``).  ``terms=True``: ``(value, means)`` with means float64 ``[5, N, C]`` — contrast-structure at scales 0 .. 3,
    SSIM at scale 4, before clipping."""
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise ValueError("ms_ssim_fused: inputs must be tensors")
    if not x.is_cuda or not y.is_cuda:
        raise _lib.GsvcError("ms_ssim_fused runs on the HIP kernels of csrc/metrics.hip; CPU tensors are not supported")
    if x.dim() == 3:
        x, y = x.unsqueeze(0), y.unsqueeze(0) if y.dim() == 3 else y
    if x.shape != y.shape or x.dim() != 4 or x.dtype != torch.float32 or y.dtype != torch.float32 or x.device != y.device:
        raise ValueError("ms_ssim_fused: inputs must be two float32 [N, C, H, W] tensors of the same shape on one device")
    N, C, H, W = (int(v) for v in x.shape)
    if min(H, W) <= _MS_MIN_SIDE:
        raise ValueError(f"ms_ssim_fused: image sides must exceed {_MS_MIN_SIDE} pixels for 5 scales")
    x, y = x.contiguous(), y.contiguous()
    t = _msssim_terms(x, y, N * C, H, W, (W, H * W), (W, H * W), SAMPLE_F32, 1.0).view(5, N, C)
    val = _msssim_value(t)
    val = val.mean() if size_average else val.mean(1)
    return (val, t) if terms else val


def psnr_of_sse(sse, samples, peak: float) -> torch.Tensor:
    """``10 log10(peak^2 samples / SSE)`` in float64, ``+inf`` where SSE is 0 (``samples``: a number or a tensor like ``sse``)."""
    sse = torch.as_tensor(sse).to(torch.float64)
    num = torch.as_tensor(samples, device=sse.device).to(torch.float64) * float(peak) ** 2
    return torch.where(sse > 0, 10.0 * torch.log10(num / sse.clamp(min=1.0)), torch.full_like(sse, float("inf")))


def plane_samples(H: int, W: int, fmt):
    """Samples of the three planes of a frame: (H W, chroma, chroma)."""
    px = int(H) * int(W)
    c = px // 4 if fmt.layout == "yuv420p" else px
    return (px, c, c)


def plane_names(fmt):
    return ("r", "g", "b") if fmt.layout == "rgb24" else ("y", "u", "v")


def code_metrics(a_u8, b_u8, H: int, W: int, fmt, msssim: bool = True) -> dict:
    """The numbers a video codec is judged by, on the sample codes of two frame buffers (as ``plane_sse`` takes them): a dict of
    per-frame float64 tensors ``[n]`` on their device, plus ``"peak"`` = ``2^depth - 1`` (ffmpeg's convention) and ``"sse"``, the int64
    ``[n, 3]`` sums.
      ``psnr_y`` / ``psnr_u`` / ``psnr_v`` (``psnr_r`` / ``_g`` / ``_b`` for ``rgb24``)  ``10 log10(peak^2 samples / SSE)`` of a plane, ``+inf`` for SSE 0
      ``psnr_avg``   from the SSE pooled over all samples of the frame (ffmpeg's ``average``)
      ``psnr_611``   ``yuv420p`` only: ``(6 Y + U + V) / 8`` of the frame's plane PSNRs
      ``msssim_y``   fused MS-SSIM of the Y planes read where they lie, codes / peak (``rgb24``: the mean over the three channels);
                     absent when a side is 160 pixels or less, or with ``msssim=False``"""
    H, W = int(H), int(W)
    sse = plane_sse(a_u8, b_u8, H, W, fmt)
    peak = float((1 << fmt.depth) - 1)
    names, counts = plane_names(fmt), plane_samples(H, W, fmt)
    out = {"peak": peak, "sse": sse}
    for k, name in enumerate(names):
        out[f"psnr_{name}"] = psnr_of_sse(sse[:, k], counts[k], peak)
    out["psnr_avg"] = psnr_of_sse(sse.sum(1), sum(counts), peak)
    if fmt.layout == "yuv420p":
        out["psnr_611"] = (6.0 * out["psnr_y"] + out["psnr_u"] + out["psnr_v"]) / 8.0
    if msssim and min(H, W) > _MS_MIN_SIDE:
        from .frames_out import frame_bytes
        nbytes = frame_bytes(H, W, fmt)
        a, n, sa = _frame_rows(a_u8, nbytes, fmt, "code_metrics")
        b, _, sb = _frame_rows(b_u8, nbytes, fmt, "code_metrics")
        if fmt.layout == "rgb24":
            # interleaved: the kernel reads planes, so the three channels are taken apart first (this layout is not a codec's)
            xa = a[:, :nbytes].reshape(n, H, W, 3).permute(0, 3, 1, 2).contiguous()
            xb = b[:, :nbytes].reshape(n, H, W, 3).permute(0, 3, 1, 2).contiguous()
            t = _msssim_terms(xa, xb, 3 * n, H, W, (W, H * W), (W, H * W), SAMPLE_U8, peak).view(5, n, 3)
            out["msssim_y"] = _msssim_value(t).mean(1)
        else:
            per = 2 if fmt.depth > 8 else 1          # (a deep frame's 16-bit words are read where they lie in the buffer of bytes)
            t = _msssim_terms(a, b, n, H, W, (W, sa // per), (W, sb // per), SAMPLE_U16 if per == 2 else SAMPLE_U8, peak)
            out["msssim_y"] = _msssim_value(t)
    return out


def compare_videos(path_a, path_b, W: int | None = None, H: int | None = None, fmt=None, chunk: int = 16) -> dict:
    """``code_metrics`` of two video files (``frames_in.open_video``: ``.y4m``, or raw ``.yuv`` / ``.rgb`` with ``W``, ``H``, ``fmt``), frame k
    of one against frame k of the other.  Layout, depth, size and the number of frames must agree (ValueError).  The frames are
    uploaded ``chunk`` at a time through one pinned staging buffer per file.  Returns ``{"frames", "W", "H", "format", "peak",
    "per_frame": {key: [floats]}, key: the mean over the frames (``report.evaluate``'s convention), key + "_seq": the PSNR of the SSE
    summed over the sequence (the summary line of ffmpeg's psnr filter; PSNR keys only)}``."""
    from .frames_in import open_video
    ha, fa = open_video(path_a, W, H, fmt)
    hb, fb = open_video(path_b, W, H, fmt)
    for key in ("layout", "depth", "W", "H"):
        if ha[key] != hb[key]:
            raise ValueError(f"compare_videos: {path_a} and {path_b} differ in {key} ({ha[key]} and {hb[key]})")
    if fa.shape[0] != fb.shape[0]:
        raise ValueError(f"compare_videos: {path_a} and {path_b} differ in frames ({fa.shape[0]} and {fb.shape[0]})")
    used, T, nbytes = ha["fmt"], int(fa.shape[0]), int(ha["frame_bytes"])
    H, W = int(ha["H"]), int(ha["W"])
    if T < 1:
        raise ValueError(f"compare_videos: {path_a}: no frames")
    chunk = max(1, min(int(chunk), T))
    import numpy as np
    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if dev is None:
        raise _lib.GsvcError("compare_videos runs on the HIP kernels of csrc/metrics.hip; it needs a CUDA device")
    stage = [torch.empty((chunk, nbytes), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    on_dev = [torch.empty((chunk, nbytes), dtype=torch.uint8, device=dev) for _ in range(2)]
    per, sse_total = {}, torch.zeros(3, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev)
    for i in range(0, T, chunk):
        m = min(chunk, T - i)
        for st, dv, src in zip(stage, on_dev, (fa, fb)):
            np.copyto(st.numpy()[:m], src[i:i + m])
            dv[:m].copy_(st[:m], non_blocking=True)
        r = code_metrics(on_dev[0][:m], on_dev[1][:m], H, W, used)
        sse_total += r["sse"].sum(0)
        for k, v in r.items():
            if k not in ("peak", "sse"):
                per.setdefault(k, []).extend(v.tolist())          # (synchronises: the staging buffers are free again)
        stream.synchronize()
    peak = float((1 << used.depth) - 1)
    out = {"frames": T, "W": W, "H": H, "format": used.name, "peak": peak, "per_frame": per}
    for k, v in per.items():
        out[k] = float(np.mean(np.asarray(v, np.float64)))
    names, counts = plane_names(used), plane_samples(H, W, used)
    for k, name in enumerate(names):
        out[f"psnr_{name}_seq"] = float(psnr_of_sse(sse_total[k], counts[k] * T, peak))
    out["psnr_avg_seq"] = float(psnr_of_sse(sse_total.sum(), sum(counts) * T, peak))
    return out
