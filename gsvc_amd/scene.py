"""Where a long clip is cut into groups of pictures (GOPs): per-frame luma histograms taken by a kernel
(``metrics.plane_histograms``, csrc/scene.hip), their distance from frame to frame, the scene cuts that distance shows, and the plan
that turns cuts and a GOP length into the ``(first, count)`` ranges tools/gsvc_encode.py fits one by one.

``histogram_distance``, ``scene_cuts`` and ``plan_gops`` are host code: they need neither a GPU nor the built library.
``video_histograms`` does (no CPU fallback).
"""
from __future__ import annotations

import numpy as np

DEFAULT_CUT_THRESHOLD = 0.5
DEFAULT_MIN_GOP = 4


def _luma(h, layout: str = "yuv420p"):
    """[n, 3, 256] -> the [n, 256] counts the detector reads: plane 0 of the planar layouts, channel 1 (G) of ``rgb24``.  An
    ``[n, 256]`` array is taken as it is."""
    h = np.asarray(h)
    if h.ndim == 3:
        if h.shape[1] != 3:
            raise ValueError(f"histogram_distance: histograms are [n, 3, bins] or [n, bins] (got {h.shape})")
        h = h[:, 1 if layout == "rgb24" else 0]
    if h.ndim != 2:
        raise ValueError(f"histogram_distance: histograms are [n, 3, bins] or [n, bins] (got {h.shape})")
    return h.astype(np.int64)


def histogram_distance(h, bins: int = 64, layout: str = "yuv420p") -> np.ndarray:
    """Histograms of n frames (``[n, 3, 256]`` as ``metrics.plane_histograms`` gives them, or the luma rows ``[n, 256]``) -> float64
    ``[n - 1]``: with the 256 bins folded to ``bins`` by summing neighbours,

        d[t] = sum_b |h[t + 1, b] - h[t, b]| / (2 samples)

    in [0, 1]: 0 for two frames with the same codes in any arrangement, 1 for two frames whose codes share no bin.  The sums are exact
    integers; the one division is the last operation.  Every frame must hold the same number of samples."""
    h = _luma(h, layout)
    n, width = h.shape
    bins = int(bins)
    if bins < 1 or width % bins:
        raise ValueError(f"histogram_distance: {width} bins do not fold to {bins}")
    if n < 1:
        raise ValueError("histogram_distance: no frames")
    folded = h.reshape(n, bins, width // bins).sum(axis=2)
    samples = folded.sum(axis=1)
    if (samples != samples[0]).any() or samples[0] <= 0:
        raise ValueError("histogram_distance: every frame must hold the same, positive number of samples")
    return np.abs(folded[1:] - folded[:-1]).sum(axis=1).astype(np.float64) / (2.0 * float(samples[0]))


def scene_cuts(d, threshold: float = DEFAULT_CUT_THRESHOLD, min_gop: int = 1) -> list:
    """Distances ``d[t]`` between frames t and t + 1 -> the frames that start a scene: ``t + 1`` wherever ``d[t] > threshold``, in
    ascending order.  ``min_gop`` > 1 drops a cut that follows the previous kept cut (or frame 0) by fewer than ``min_gop`` frames
    (``plan_gops`` merges short scenes itself; this only thins a list that is looked at).

    The default threshold 0.5 is a starting value that nobody has measured on real content: it separates the synthetic clips of the
    tests (whose cuts have distance 1 and whose motion stays below 0.25) and nothing more is claimed for it."""
    d = np.asarray(d, np.float64).reshape(-1)
    cuts, last = [], 0
    for t in np.nonzero(d > float(threshold))[0].tolist():
        if t + 1 - last >= int(min_gop):
            cuts.append(t + 1)
            last = t + 1
    return cuts


def plan_gops(T: int, cuts=(), gop_frames: int = 32, min_gop: int = DEFAULT_MIN_GOP) -> list:
    """The GOPs of a clip of ``T`` frames as ``[(first, count)]``, tiling ``[0, T)``.  Pure and deterministic.
      1. Scenes are the intervals between ``cuts`` (frames that start a scene; 0, duplicates and anything outside (0, T) are ignored).
      2. Left to right, a scene shorter than ``min_gop`` joins the previous scene; the first joins the next.
      3. A scene of length L becomes k = ceil(L / gop_frames) GOPs whose lengths differ by at most one, the longer ones first.
    ``min_gop >= 2`` (a training step reads frames i and i + 1) and ``gop_frames >= 2 min_gop``: every GOP then has between ``min_gop``
    and ``gop_frames`` frames, unless ``T < min_gop``, which gives the one GOP ``(0, T)``."""
    T, gop_frames, min_gop = int(T), int(gop_frames), int(min_gop)
    if T < 1:
        raise ValueError(f"plan_gops: a clip has at least one frame (got {T})")
    if min_gop < 2:
        raise ValueError(f"plan_gops: min_gop must be at least 2 (got {min_gop})")
    if gop_frames < 2 * min_gop:
        raise ValueError(f"plan_gops: gop_frames must be at least 2 x min_gop = {2 * min_gop} (got {gop_frames})")
    starts = [0] + sorted({int(c) for c in cuts if 0 < int(c) < T})
    lengths = [b - a for a, b in zip(starts, starts[1:] + [T])]
    merged = []
    for L in lengths:
        if merged and (L < min_gop or merged[-1] < min_gop):          # (merged[-1] < min_gop: only a too-short FIRST scene is left open)
            merged[-1] += L
        else:
            merged.append(L)
    out, at = [], 0
    for L in merged:
        k = -(-L // gop_frames)
        base, longer = divmod(L, k)
        for i in range(k):
            count = base + (1 if i < longer else 0)
            out.append((at, count))
            at += count
    assert at == T
    return out


def gop_cut_flags(gops, cuts) -> list:
    """1 for a GOP that starts at one of ``cuts``, else 0."""
    at = {int(c) for c in cuts}
    return [1 if first in at and first > 0 else 0 for first, _ in gops]


def _opened(video):
    """A path ``frames_in.open_video`` reads, or its ``(header, frames)`` -> ``(header, frames)``."""
    if isinstance(video, (str, bytes)) or hasattr(video, "__fspath__"):
        from .frames_in import open_video
        return open_video(video)
    return video


def video_histograms(video, device="cuda", chunk: int = 16):
    """The histograms of every frame of a video file (a path ``frames_in.open_video`` reads, or its ``(header, frames)``) -> int32
    ``[T, 3, 256]`` on the HOST (a numpy array).  The frames are uploaded ``chunk`` at a time through one pinned staging buffer, as
    ``VideoFileCube`` uploads them, and each chunk is reduced by one launch of ``metrics.plane_histograms``: the video is never resident
    as a whole, on the device it costs ``chunk`` frames and 3 KB per frame."""
    import torch

    from . import _lib
    from .metrics import plane_histograms
    header, frames = _opened(video)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.GsvcError("video_histograms runs on the HIP kernels of csrc/scene.hip; it needs a CUDA device")
    T, H, W, fmt, nbytes = int(frames.shape[0]), int(header["H"]), int(header["W"]), header["fmt"], int(header["frame_bytes"])
    if T < 1:
        raise ValueError("video_histograms: no frames")
    chunk = max(1, min(int(chunk), T))
    staging = torch.empty((chunk, nbytes), dtype=torch.uint8, pin_memory=True)
    host = staging.numpy()
    out = torch.empty((T, 3, 256), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        on_dev = torch.empty((chunk, nbytes), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        for i in range(0, T, chunk):
            m = min(chunk, T - i)
            np.copyto(host[:m], frames[i:i + m])
            on_dev[:m].copy_(staging[:m], non_blocking=True)
            out[i:i + m] = plane_histograms(on_dev[:m], H, W, fmt)
            stream.synchronize()          # the staging buffer is free again
    return out.cpu().numpy()


def detect_cuts(video, device="cuda", threshold: float = DEFAULT_CUT_THRESHOLD, bins: int = 64):
    """``video_histograms`` -> ``histogram_distance`` -> ``scene_cuts``: ``(cuts, d)`` of a video file."""
    header, frames = _opened(video)
    if int(frames.shape[0]) < 2:
        return [], np.zeros(0, np.float64)
    d = histogram_distance(video_histograms((header, frames), device), bins=bins, layout=header["fmt"].layout)
    return scene_cuts(d, threshold), d
