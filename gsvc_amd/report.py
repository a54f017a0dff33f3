"""Evaluation loop and checkpoints (harness around the hot path).

``evaluate`` reports what reference utils/report_utils.py:268-390 logs for a fitted model — mean L1, PSNR, SSIM and MS-SSIM
of the two-view frames against the ground truth, and the frame rate — but renders through the decoder loop
(``render_frames``: batched generation, one two-view pass per frame) instead of two ``render`` calls, a flip and an
average per frame.  LPIPS (``lpips_fn``: gsvc_amd.lpips.LPIPS built from a weights file — the pretrained numbers are not in this
image) is reported when handed in, as the reference calls it (``lpips_fn(image, gt, normalize=True)``, report_utils.py:154).  ``save_checkpoint`` / ``load_checkpoint`` keep a model and
its optimizer in one ``torch.save`` file (the reference scatters this over ply / pkl files with third-party readers).
"""
from __future__ import annotations

import time

import torch

from .loss_utils import l1_loss_func, psnr_func, ssim_func
from .metrics import msssim_fn
from .ortho_gaussian_renderer import render_frames


@torch.no_grad()
def evaluate(pc, dataset, pipe, bg_color, frame_ids=None, batch: int = 8, lpips_fn=None, eight_bit: bool = False, delivered=None,
             code_metrics: bool = False, source_u8=None, msssim: str = "torch", weight_maps=None, weight_cell=None) -> dict:
    """Mean L1 / PSNR / SSIM / MS-SSIM (MS-SSIM only for frames at least 160 pixels high and large enough for 5 scales) of the
    rendered two-view frames, clamped to [0, 1], against ``dataset[i].image``; ``fps`` counts the whole loop's wall time,
    metrics excluded.  ``eight_bit=True``: the metrics are taken on what the decoder delivers — the frames quantised to 8 bits
    (``frames_out.frames_to_u8``: rgb24, truncating, as the reference's PNGs) / 255 — as a codec's PSNR is, and the result says so
    (``"eight_bit": True``).  ``delivered=FrameFormat(...)``: the metrics are taken on ``frames_out.delivered_images`` of the frames —
    what a viewer of frames delivered in that format sees, at its depth and chroma subsampling — and the result records the format
    (``"delivered": fmt.name``).  Giving both is a ValueError.
    ``code_metrics=True`` (needs ``delivered=fmt``) adds what a video codec is judged by, taken on the sample codes
    (``metrics.code_metrics``) between ``frames_to_u8(rendered, fmt)`` and the source's frames in ``fmt`` — ``source_u8`` when given (uint8
    ``[frames, frame_bytes]``, tensor or array, in the order of ``frame_ids``: for example a file's own bytes from ``open_video``), else
    ``frames_to_u8(gt, fmt)``: ``psnr_y``, ``psnr_u``, ``psnr_v``, ``psnr_avg``, ``psnr_611`` (``yuv420p``) and ``msssim_y`` (frames with both sides above
    160 pixels), each the mean over the frames.  ``msssim="fused"``: the ``msssim`` entry comes from ``metrics.ms_ssim_fused`` instead of
    the tensor expressions.  ``weight_maps`` (``[T, Hc, Wc]`` for the dataset's frames at ``weight_cell``, gsvc_amd/wdist.py; needs
    ``code_metrics=True`` and a Y'CbCr ``delivered``): adds ``wpsnr_y``, the mean over the frames of ``wdist.weighted_psnr_y`` under each
    frame's own map, on the same codes as ``psnr_y``."""
    if weight_maps is not None and (not code_metrics or delivered is None or delivered.layout == "rgb24" or weight_cell is None):
        raise ValueError("evaluate: weight_maps needs code_metrics=True, a Y'CbCr delivered= format and weight_cell")
    if eight_bit and delivered is not None:
        raise ValueError("evaluate: eight_bit=True and delivered= both say what is delivered; give one")
    if code_metrics and delivered is None:
        raise ValueError("evaluate: code_metrics=True compares frames of codes; say which with delivered=FrameFormat(...)")
    if source_u8 is not None and not code_metrics:
        raise ValueError("evaluate: source_u8 is the source of code_metrics=True")
    if msssim not in ("torch", "fused"):
        raise ValueError(f"evaluate: msssim must be 'torch' or 'fused' (got {msssim!r})")
    ids = list(range(dataset.len_z_frames)) if frame_ids is None else list(frame_ids)
    frames = [dataset[i] for i in ids]
    for _ in render_frames(frames[:min(len(frames), batch)], pc, pipe, bg_color, batch=batch):      # warm-up, as the reference does
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    images = [torch.clamp(img, 0.0, 1.0) for img in render_frames(frames, pc, pipe, bg_color, batch=batch)]
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if eight_bit and images:
        from .frames_out import FrameFormat, frames_to_u8, rgb24_to_image
        H, W = images[0].shape[1:]
        images = [rgb24_to_image(u8, H, W) for u8 in frames_to_u8(images, FrameFormat("rgb24", rounding="trunc"))]
    rendered = images
    if delivered is not None and images:
        from .frames_out import delivered_images
        images = list(delivered_images(images, delivered).unbind(0))
    sums = {"l1": 0.0, "psnr": 0.0, "ssim": 0.0, "msssim": 0.0, "lpips": 0.0}
    n_ms = 0
    gts = []
    for fr, img in zip(frames, images):
        gt = torch.clamp(fr.image.to(img.device), 0.0, 1.0).permute(0, 2, 1).contiguous()
        if code_metrics and source_u8 is None:
            gts.append(gt)
        sums["l1"] += float(l1_loss_func(img, gt).mean())
        sums["psnr"] += float(psnr_func(img, gt))
        sums["ssim"] += float(ssim_func(img, gt).mean())
        if min(img.shape[-2:]) > 160:
            if msssim == "fused":
                from .metrics import ms_ssim_fused
                sums["msssim"] += float(ms_ssim_fused(img.float().detach(), gt.detach()))
            else:
                sums["msssim"] += float(msssim_fn(img.unsqueeze(0), gt.unsqueeze(0)))
            n_ms += 1
        if lpips_fn is not None:
            sums["lpips"] += float(lpips_fn(img, gt, normalize=True))
    n = max(len(frames), 1)
    out = {"frames": len(frames), "l1": sums["l1"] / n, "psnr": sums["psnr"] / n, "ssim": sums["ssim"] / n,
           "msssim": sums["msssim"] / n_ms if n_ms else float("nan"), "lpips": sums["lpips"] / n if lpips_fn is not None else None, "fps": len(frames) / elapsed if elapsed > 0 else float("inf")}
    if eight_bit:
        out["eight_bit"] = True
    if delivered is not None:
        out["delivered"] = delivered.name
    if code_metrics and rendered:
        weights = None if weight_maps is None else (weight_maps[ids], int(weight_cell))
        out.update(_code_metrics_means(rendered, gts, source_u8, delivered, batch, weights))
    return out


def _code_metrics_means(rendered, gts, source_u8, fmt, batch, weights=None):
    """Means over the frames of ``metrics.code_metrics`` between the rendered frames' codes and the source's (see ``evaluate``);
    ``weights = (maps [frames, Hc, Wc], cell)``: also of the weighted luma PSNR."""
    from .frames_out import frame_bytes, frames_to_u8
    from .metrics import code_metrics
    H, W = (int(v) for v in rendered[0].shape[1:])
    nbytes, dev = frame_bytes(H, W, fmt), rendered[0].device
    if source_u8 is not None:
        import numpy as np
        src = source_u8 if isinstance(source_u8, torch.Tensor) else torch.from_numpy(np.array(source_u8))      # (a copy: a memory map may be read-only)
        if src.dtype != torch.uint8 or src.dim() != 2 or src.shape[0] != len(rendered) or src.shape[1] < nbytes:
            raise ValueError(f"evaluate: source_u8 must be uint8 [{len(rendered)}, >= {nbytes}] (got {src.dtype} {tuple(src.shape)})")
        src = src.to(dev)
    sums = {}
    step = max(int(batch), 1)
    for i in range(0, len(rendered), step):
        dec = frames_to_u8(rendered[i:i + step], fmt)
        ref = src[i:i + step] if source_u8 is not None else frames_to_u8(gts[i:i + step], fmt)
        for k, v in code_metrics(dec, ref, H, W, fmt).items():
            if k not in ("peak", "sse"):
                sums[k] = sums.get(k, 0.0) + float(v.sum())
        if weights is not None:
            from .wdist import block_sse, weighted_psnr_y
            per, _ = weighted_psnr_y(block_sse(dec, ref, H, W, fmt, weights[1]), weights[0][i:i + step], fmt.depth, H, W)
            sums["wpsnr_y"] = sums.get("wpsnr_y", 0.0) + float(per.sum())
    return {k: v / len(rendered) for k, v in sums.items()}


def _optimizer_state(optimizer):
    return optimizer.state_dict()


def _plain(obj):
    """NumPy scalars -> Python numbers, recursively (the learning-rate schedule leaves np.float64 in the optimizer's groups;
    a file holding them cannot be read back with ``weights_only=True``)."""
    import numpy as np
    if isinstance(obj, dict):
        return {k: _plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_plain(v) for v in obj)
    if isinstance(obj, np.generic):
        return obj.item()
    return obj


def save_checkpoint(pc, path, iteration: int = 0):
    """Model parameters (reference-compatible state_dict keys), the per-anchor tensors, the densification statistics and
    the optimizer state in one file."""
    per_anchor = {n: getattr(pc, n).detach() for n in ("_anchor", "_offset", "_mask", "_anchor_feat", "_scaling", "_rotation", "_opacity")}
    stats = {n: getattr(pc, n) for n in ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom", "max_radii2D")}
    torch.save({"iteration": int(iteration), "state_dict": pc.state_dict(), "per_anchor": per_anchor, "stats": stats,
                "decoded_version": bool(pc.decoded_version), "voxel_size": float(pc.voxel_size),
                "spatial_lr_scale": float(pc.spatial_lr_scale), "percent_dense": float(getattr(pc, "percent_dense", 0.0) or 0.0),
                "bounds": (tuple(float(v) for v in pc.bound_min_host), tuple(float(v) for v in pc.bound_max_host)),
                "optimizer": _plain(_optimizer_state(pc.optimizer)) if pc.optimizer is not None else None}, path)


def load_checkpoint(pc, path, training_args=None) -> int:
    """Restore what save_checkpoint wrote into a model built with the same hyper-parameters; with ``training_args`` the
    optimizer is set up and its state restored.  Returns the stored iteration."""
    ck = torch.load(path, map_location=pc.device, weights_only=True)      # tensors / numbers / tuples only: nothing is unpickled
    for n, t in ck["per_anchor"].items():
        setattr(pc, n, torch.nn.Parameter(t.to(pc.device).clone(), requires_grad=n not in ("_rotation", "_opacity")))
    pc.load_state_dict(ck["state_dict"], strict=True)
    pc.decoded_version, pc.voxel_size = ck["decoded_version"], ck["voxel_size"]
    lo, hi = ck["bounds"]
    pc.bound_min_host, pc.bound_max_host = tuple(lo), tuple(hi)
    pc.x_bound_min = torch.tensor([list(lo)], dtype=torch.float32, device=pc.device)
    pc.x_bound_max = torch.tensor([list(hi)], dtype=torch.float32, device=pc.device)
    pc.spatial_lr_scale = float(ck.get("spatial_lr_scale", pc.spatial_lr_scale))
    if training_args is not None:
        pc.training_setup(training_args)      # re-creates (zeroes) the densification statistics: restore them afterwards
        if ck["optimizer"] is not None:
            pc.optimizer.load_state_dict(ck["optimizer"])
    if ck.get("percent_dense"):
        pc.percent_dense = float(ck["percent_dense"])
    for n, t in ck["stats"].items():
        setattr(pc, n, t.to(pc.device) if isinstance(t, torch.Tensor) else t)
    return ck["iteration"]
