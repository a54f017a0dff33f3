"""Lanczos-3 resampler on the codes of planar Y'CbCr frames (host side of csrc/resample.hip).

Nothing else in this project changes a picture's size.  AV1 (super-resolution, reference scaling) and VVC (RPR) code a reduced
picture and let the decoder bring it back to display size, because at low rates the coded picture cannot carry the source's
pixel-level detail anyway; here the fit's time, the anchor count and the model's bits all grow with the pixel count.
``encode_gop(coded_size=...)`` fits the resampled source and writes the display size into the file (section DISP);
``decode_video(size=...)`` resamples the decoded pictures on the device, to the display size or to any preview size;
``resample_video`` / tools/scale_video.py prepare sources.  Whether a smaller coded picture pays is an experiment per clip.

The resampler, exactly
----------------------
Formats.  Planar ``yuv420p`` / ``yuv444p`` at depth 8, 10, 12 or 16 (``rgb24`` raises ``ValueError``).  Every plane is resampled on its
own, between its own dimensions: in 4:2:0 the chroma planes go from ``(H / 2, W / 2)`` to ``(H' / 2, W' / 2)`` (all four sizes even).
The mapping is centre-aligned on every plane, which keeps centre-sited chroma centre-sited.  Each side satisfies ``src <= 4 dst`` and
``dst <= 4 src`` and is at least 2 (so a chroma side is at least 1).

Taps (``filter_taps(src, dst)``; numpy float64 on the host, no GPU and no library).  ``//`` is floor division.  For output index ``j``
let ``M = max(src, dst)`` and ``P = (2 j + 1) src - dst``: the centre of output sample ``j`` lies at ``P / (2 dst)`` in source
coordinates.  The taps are the source indices ``i`` with ``|2 dst i - P| < 6 M``:

    lo = (P - 6 M) // (2 dst) + 1,      hi = -((-(P + 6 M)) // (2 dst)) - 1          (at most 24 within the ratio limit)

and their weights are formed in this order:

    1. w_i = L((2 dst i - P) / (2 M)),   L(0) = 1,  L(x) = 3 sin(pi x) sin(pi x / 3) / (pi^2 x^2) for |x| < 3
       (Lanczos-3, widened by the downscale ratio so that it antialiases)
    2. w /= sum w
    3. c = rint(16384 w)
    4. c[first index of max(c)] += 16384 - sum c

stored as ``first[j] = lo`` and ``coef[j, :count] = c`` with zeros behind; ``nt`` is the largest count of the table.  The builder
asserts ``sum |c| <= 32767`` for every row (the largest value seen is 25 288).  The tables come from libm's ``sin``: two hosts could in
principle differ in the last bit of a coefficient, which is why a file's picture hashes stay those of the CODED picture.

Arithmetic.  All integers; ``>>`` is the arithmetic shift; ``d`` is the depth; every tap index is clamped into the plane,
``clamp(first + k, 0, src - 1)``.

    horizontal, over the source rows     t(y, j) = sum_k cx[j, k] a(y, clamp(fx[j] + k))                 |t| < 2^31
                                         m       = (t + 2^(d - 3)) >> (d - 2)                            not clamped, |m| < 2^17
    vertical                             u(i, j) = sum_k cy[i, k] m(clamp(fy[i] + k), j)                 exact, |u| < 2^33
                                         out     = clamp((u + 2^(29 - d)) >> (30 - d), 0, 2^d - 1)

The intermediate is deliberately not clamped: clamped to the code range between the passes, full-range noise moved by up to 30 codes at
8 bits against the float64 filter; unclamped the difference is rounding only.  An axis with ``src == dst`` has one coefficient of 16384
per row, so a 1:1 call returns the input bytes at every depth, and a constant plane stays constant.  Codes are read as they are: a word
above ``2^d - 1`` in a deep frame is not masked (the bounds above then do not hold, but the sums still fit 64 bits).

Importing this module needs neither a GPU nor the built library; ``resample_frames`` and what is built on it do (no CPU fallback).
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib
from .frames_out import LAYOUTS, MAX_BATCH, FrameFormat, frame_bytes

TAPS = 24                    # GSVC_RESAMPLE_TAPS: slots per coefficient row
MAX_RATIO = 4
ONE = 16384                  # Q14
FILTER_IDS = {1: "lanczos3"}          # the filter ids of the bitstream's DISP section


def check_side(src: int, dst: int, what: str, axis: str = "side"):
    """The ratio limit and the minimum of one side of a plane."""
    if src < 2 or dst < 2:
        raise ValueError(f"{what}: a {axis} must be at least 2 (got {src} -> {dst})")
    if src > MAX_RATIO * dst or dst > MAX_RATIO * src:
        raise ValueError(f"{what}: a {axis} changes by a ratio of at most {MAX_RATIO} either way (got {src} -> {dst})")


def check_sizes(H: int, W: int, out_H: int, out_W: int, fmt: FrameFormat, what: str):
    """Everything ``resample_frames`` refuses about formats and sizes, as ``ValueError``."""
    if fmt.layout == "rgb24":
        raise ValueError(f"{what}: rgb24 frames are not resampled; the filter works on planar Y'CbCr codes")
    if fmt.depth not in (8, 10, 12, 16):
        raise ValueError(f"{what}: depth must be 8, 10, 12 or 16 (got {fmt.depth})")
    if fmt.layout == "yuv420p" and (H % 2 or W % 2 or out_H % 2 or out_W % 2):
        raise ValueError(f"{what}: yuv420p needs even sizes (got {W} x {H} -> {out_W} x {out_H})")
    check_side(H, out_H, what, "height")
    check_side(W, out_W, what, "width")


def lanczos3(x):
    """``L(x)`` of the module's docstring for a float64 array: 1 at 0, 0 from ``|x| = 3`` on."""
    x = np.asarray(x, np.float64)
    safe = np.where(x == 0.0, 1.0, x)
    v = 3.0 * np.sin(math.pi * safe) * np.sin(math.pi * safe / 3.0) / (math.pi * math.pi * safe * safe)
    return np.where(x == 0.0, 1.0, np.where(np.abs(x) < 3.0, v, 0.0))


def tap_range(src: int, dst: int, j: int):
    """``(lo, hi, P, M)`` of output index ``j``: the taps are the source indices ``lo .. hi`` (before clamping)."""
    M = max(src, dst)
    P = (2 * j + 1) * src - dst
    return (P - 6 * M) // (2 * dst) + 1, -((-(P + 6 * M)) // (2 * dst)) - 1, P, M


def filter_weights(src: int, dst: int, j: int):
    """``(lo, w)``: the normalised float64 weights of output index ``j`` before they are quantised (steps 1 and 2)."""
    lo, hi, P, M = tap_range(src, dst, j)
    i = np.arange(lo, hi + 1, dtype=np.int64)
    w = lanczos3((2 * dst * i - P).astype(np.float64) / float(2 * M))
    return lo, w / w.sum()


def filter_taps(src: int, dst: int):
    """The table of one axis: ``(first int32 [dst], coef int16 [dst, 24], nt)`` as the module's docstring states it."""
    src, dst = int(src), int(dst)
    if src < 1 or dst < 1 or src > MAX_RATIO * dst or dst > MAX_RATIO * src:
        raise ValueError(f"filter_taps: sizes must be positive and within a ratio of {MAX_RATIO} (got {src} -> {dst})")
    first = np.zeros(dst, np.int32)
    coef = np.zeros((dst, TAPS), np.int16)
    nt = 0
    for j in range(dst):
        lo, w = filter_weights(src, dst, j)
        c = np.rint(ONE * w).astype(np.int64)
        c[int(np.argmax(c))] += ONE - int(c.sum())
        assert len(c) <= TAPS, (src, dst, j, len(c))
        assert int(np.abs(c).sum()) <= 32767, (src, dst, j, int(np.abs(c).sum()))
        first[j] = lo
        coef[j, :len(c)] = c
        nt = max(nt, len(c))
    return first, coef, nt


# ----------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------
_TABLES: dict = {}          # (src, dst, device) -> (first int32 [dst], coef int16 [dst, 24], nt) on the device


def device_taps(src: int, dst: int, device):
    """``filter_taps(src, dst)`` as device arrays, built once per ``(src, dst)`` and device."""
    import torch
    dev = torch.device(device)
    key = (int(src), int(dst), dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    hit = _TABLES.get(key)
    if hit is None:
        first, coef, nt = filter_taps(src, dst)
        hit = _TABLES[key] = (torch.from_numpy(first).to(dev), torch.from_numpy(coef).to(dev), nt)
    return hit


def resample_frames(frames_u8, H: int, W: int, fmt: FrameFormat, out_H: int, out_W: int, out=None):
    """Frames of ``fmt`` (uint8 CUDA ``[n, >= frame_bytes(H, W, fmt)]`` with contiguous rows, or one flat frame; deep formats: little-endian
    16-bit samples, even base and row stride) resampled to ``out_H x out_W`` -> uint8 ``[n, frame_bytes(out_H, out_W, fmt)]`` on their
    device (``out``: given, ``[n, >= that]`` with contiguous rows, bytes of a row beyond the frame are left alone and the return value is
    its ``[:, :frame_bytes]`` view; it may not overlap the input).  Any ``n``: one launch per 16 frames on the current stream; nothing
    synchronises once the tables of this ``(size, device)`` exist."""
    import torch

    from .metrics import _frame_rows
    H, W, out_H, out_W = int(H), int(W), int(out_H), int(out_W)
    check_sizes(H, W, out_H, out_W, fmt, "resample_frames")
    in_bytes, out_bytes = frame_bytes(H, W, fmt), frame_bytes(out_H, out_W, fmt)
    a, n, stride = _frame_rows(frames_u8, in_bytes, fmt, "resample_frames")
    if out is None:
        out = torch.empty((n, out_bytes), dtype=torch.uint8, device=a.device)
    o, no, ostride = _frame_rows(out, out_bytes, fmt, "resample_frames")
    if no != n or o.device != a.device:
        raise ValueError(f"resample_frames: out must hold {n} frames on the frames' device (got {no})")
    sub = fmt.layout == "yuv420p"
    ch, cw, och, ocw = (H // 2, W // 2, out_H // 2, out_W // 2) if sub else (H, W, out_H, out_W)
    tables = []
    for s, d in ((W, out_W), (H, out_H), (cw, ocw), (ch, och)):
        first, coef, nt = device_taps(s, d, a.device)
        tables += [first.data_ptr(), coef.data_ptr(), nt]
    L = _lib.lib()
    with torch.cuda.device(a.device):
        stream = _lib.current_stream(a.device)
        for i in range(0, n, MAX_BATCH):
            m = min(MAX_BATCH, n - i)
            _lib.check(L.gsvc_resample_frames(a.data_ptr() + i * stride, stride, m, H, W, LAYOUTS[fmt.layout], fmt.depth,
                                              o.data_ptr() + i * ostride, ostride, out_H, out_W, *tables, stream), "gsvc_resample_frames")
    return o[:, :out_bytes]


def resample_range(frames_host, H: int, W: int, fmt: FrameFormat, out_H: int, out_W: int, device):
    """``resample_frames`` of a host array ``[T, frame_bytes]`` -> uint8 numpy ``[T, frame_bytes(out_H, out_W, fmt)]``: uploaded, resampled
    and downloaded in chunks of 16."""
    import torch
    dev = torch.device(device)
    check_sizes(int(H), int(W), int(out_H), int(out_W), fmt, "resample_range")
    T = int(frames_host.shape[0])
    res = np.empty((T, frame_bytes(out_H, out_W, fmt)), np.uint8)
    with torch.cuda.device(dev):
        for i in range(0, T, MAX_BATCH):
            up = torch.from_numpy(np.ascontiguousarray(frames_host[i:i + MAX_BATCH])).to(dev)
            res[i:i + MAX_BATCH] = resample_frames(up, H, W, fmt, out_H, out_W).cpu().numpy()
    return res


def resample_video(src_path, dst_path, size, W: int | None = None, H: int | None = None, fmt: FrameFormat | None = None,
                   device="cuda") -> dict:
    """File to file: the frames of ``src_path`` (``frames_in.open_video``) resampled to ``size = (W', H')`` and written to ``dst_path``
    (``frames_out.open_sink``) in the source's own format.  Returns {"W", "H", "frames", "format", "source_W", "source_H"}."""
    from .frames_in import open_video
    from .frames_out import open_sink
    hdr, frames = open_video(src_path, W, H, fmt)
    used = hdr["fmt"]
    Wf, Hf, T = int(hdr["W"]), int(hdr["H"]), int(frames.shape[0])
    Wo, Ho = parse_size(size) if isinstance(size, str) else (int(size[0]), int(size[1]))
    check_sizes(Hf, Wf, Ho, Wo, used, "resample_video")
    sink, _ = open_sink(dst_path, Wo, Ho, hdr.get("fps") or (30, 1), used)
    with sink:
        for i in range(0, T, MAX_BATCH):
            for row in resample_range(frames[i:i + MAX_BATCH], Hf, Wf, used, Ho, Wo, device):
                sink.write(row)
    return {"W": Wo, "H": Ho, "frames": T, "format": used.name, "source_W": Wf, "source_H": Hf}


def parse_size(text):
    """The ``type=`` of a ``WxH`` command-line option (``--size`` of tools/scale_video.py, ``--coded-size`` of tools/gsvc_encode.py):
    ``(W, H)`` as two positive ints; anything else is an ``argparse.ArgumentTypeError``."""
    import argparse
    parts = str(text).lower().split("x")
    try:
        w, h = (int(v) for v in parts)
    except ValueError:
        w = h = 0
    if len(parts) != 2 or w < 1 or h < 1:
        raise argparse.ArgumentTypeError(f"a size WxH of two positive integers is expected (got {text!r})")
    return w, h


def parse_decode_size(text):
    """The ``type=`` of ``--size {display,coded,WxH}`` of tools/gsvc_decode.py: the word, or ``(W, H)``."""
    return text if text in ("display", "coded") else parse_size(text)
