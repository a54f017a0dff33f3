"""Motion-compensated temporal prefilter of the encoder's source frames (host side of csrc/tfilter.hip).

Production encoders denoise the source before coding it (MCTF in VTM and x265, temporal filtering in SVT-AV1 and libaom, where it is
the analysis half of the film-grain tool).  A splat model at 0.06 - 0.10 bpp cannot represent sensor noise (gsvc_amd/grain.py), yet the
fit spends densification and gradient on it.  ``denoise_frames`` filters one resident GOP along the motion ``flow.estimate_flow``
finds between its frames; the result is a video in the same ``FrameFormat`` and everything downstream takes it unchanged.  With
``film_grain`` the grain statistics stay measured against the ORIGINAL source, so what the filter removed is what the decoder puts
back.  Opt-in (``encode_gop(denoise=...)``, ``--denoise``); whether a fit gains from it is an experiment, not a known result.

The filter, exactly
-------------------
Everything is an integer; ``//`` is floor division; all sums are exact.

Inputs.  ``T`` frames of a planar ``yuv420p`` / ``yuv444p`` format at depth 8, 10, 12 or 16 (``rgb24`` raises ``ValueError``), ``H, W >= 8``.
For each target frame ``t`` and each offset ``d`` in (-2, -1, +1, +2) with ``0 <= t + d < T`` a float32 flow ``[2, H, W]`` from frame ``t`` to
frame ``t + d`` in the convention of flow.py, ``I_t(x, y) ~ I_{t+d}(x + f[0], y + f[1])``.  Neighbours outside ``0 .. T - 1`` do not exist and
contribute nothing: the caller passes one GOP, so the filter never looks across a scene cut.

Vectors.  ``mv = clamp(rint(4 f), -32768, 32767)`` per component, the float32 product rounded half to even: quarter luma pels.  Flows
must be finite for the result to mean anything.  Every sampled position is clamped into its plane (below), so no flow value can make the
kernel read outside a frame: +-inf clamps like any large value and the kernel reads a NaN component as -32768 (its ``fmax`` / ``fmin``
return the number).  Nothing checks the flows: those of ``estimate_flow`` are finite.

Prediction.  For a plane of ``h x w`` samples with ``unit`` sub-positions per sample:

    px   = clamp(unit x + mvx, 0, unit (w - 1)),      py likewise
    x0   = min(px // unit, w - 2),   fx = px - unit x0,      y0, fy likewise
    pred = ((unit - fx)(unit - fy) a00 + fx (unit - fy) a01 + (unit - fx) fy a10 + fx fy a11 + unit^2 / 2) // unit^2

over the four codes ``a00 = a(y0, x0)``, ``a01 = a(y0, x0 + 1)``, ``a10 = a(y0 + 1, x0)``, ``a11`` of frame ``t + d``.  Luma and 4:4:4 chroma:
``unit = 4`` with the ``mv`` of the pixel itself.  4:2:0 chroma: ``unit = 8`` with the ``mv`` of luma pixel ``(2y, 2x)``: the same integers, read
as eighths of a chroma sample.

Weights.  ``q[p] >= 1`` is the noise strength of plane ``p`` in sixteenths of a code at the format's depth.  The luma plane is cut into
8 x 8 blocks; partial blocks at the right and bottom edges count the ``n_B`` pixels they have.  Per block ``B`` and neighbour ``d``, and
per sample of plane ``p``:

    SSE = sum over B of (Y_t - pred_d)^2,      i_b = min(63, 2048 SSE // (n_B q[0]^2))
    i_p = min(63, 128 |c - pred_d| // q[p])
    w_d = (wt[|d| - 1] LUT_B[i_b] LUT_P[i_p] + 2^15) >> 16

For a chroma sample ``i_b`` is that of the luma block holding ``(2y, 2x)`` (4:4:4: the block holding ``(y, x)``).

Output.  ``out = (256 c + sum_d w_d pred_d + Wt // 2) // Wt`` with ``Wt = 256 + sum_d w_d``: a weighted mean of in-range codes, so no clamp is
needed.

Defaults.  ``wt = (128, 64)``, ``LUT_B[i] = rint(256 exp(-max(0, i - 16) / 8))``, ``LUT_P[i] = rint(256 exp(-(i / 8)^2 / 18))`` for
``i = 0 .. 63`` (``default_luts``: float64 on the host, handed to the library as 64 uint16 each).  ALL of these are starting values nobody
has measured on camera material.  ``wt = (0, 0)`` returns the input bytes.

Range.  ``q <= 65535``; ``wt`` and every table entry ``<= 256``, so a weight is at most 256.  With that every intermediate fits in 64 bits (the
largest is ``2048 SSE < 2^50``), and everything per sample fits in 32 bits apart from the block sum.

The noise estimate, exactly
---------------------------
Immerkaer's estimator on the codes, per frame and plane (``noise_sums`` -> exact int64 ``[n, 3]``): ``S`` is the sum over the interior
samples ``1 <= y <= h - 2, 1 <= x <= w - 2`` of the plane of

    |c(y-1,x-1) - 2 c(y-1,x) + c(y-1,x+1) - 2 c(y,x-1) + 4 c(y,x) - 2 c(y,x+1) + c(y+1,x-1) - 2 c(y+1,x) + c(y+1,x+1)|

and on the host (``noise_strength``) ``sigma[p] = sqrt(pi / 2) sum S / (6 sum of interior samples)`` over the frames given and
``q[p] = clamp(round(16 gain sigma[p]), 1, 65535)``.  The estimator reads texture as noise: its value is a starting value.

Importing this module needs neither a GPU nor the built library; the kernels do (no CPU fallback).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from .frames_out import LAYOUTS, MAX_BATCH, FrameFormat, frame_bytes

OFFSETS = (-2, -1, 1, 2)            # the neighbour of flow slot 0 .. 3
LUT_SIZE = 64
WEIGHT_MAX = 256                    # of wt[] and of a table entry
Q_MAX = 65535
DEFAULT_WT = (128, 64)              # the weight of a neighbour at distance 1, 2 (of 256 for the frame itself).  Starting values, not measured


def default_luts():
    """``(LUT_B, LUT_P)``: two tuples of 64 ints, computed in float64.  With sigma = q / 16 codes, i_b is 8 MSE / sigma^2 of the block and
    i_p is 8 |c - pred| / sigma: LUT_B keeps a block at full weight up to an MSE of 2 sigma^2 (what two noisy pictures of the same
    content differ by) and falls by e per sigma^2 beyond, LUT_P is a Gaussian of standard deviation 3 sigma in the sample's own
    difference.  Both are starting values nobody has measured on camera material."""
    lut_b = tuple(int(np.rint(256.0 * math.exp(-max(0, i - 16) / 8.0))) for i in range(LUT_SIZE))
    lut_p = tuple(int(np.rint(256.0 * math.exp(-((i / 8.0) ** 2) / 18.0))) for i in range(LUT_SIZE))
    return lut_b, lut_p


@dataclass(frozen=True)
class TemporalFilterParams:
    """The weights of the filter (the module's docstring says what each does): ``wt`` (distance 1, distance 2), the two tables of 64
    entries, all 0 .. 256, and ``radius``, which is 2.  None for a table: that of ``default_luts``."""
    wt: tuple = DEFAULT_WT
    lut_b: tuple | None = None
    lut_p: tuple | None = None
    radius: int = 2

    def __post_init__(self):
        b, p = default_luts()
        object.__setattr__(self, "wt", tuple(int(v) for v in self.wt))
        object.__setattr__(self, "lut_b", tuple(int(v) for v in (b if self.lut_b is None else self.lut_b)))
        object.__setattr__(self, "lut_p", tuple(int(v) for v in (p if self.lut_p is None else self.lut_p)))
        if int(self.radius) != 2:
            raise ValueError(f"TemporalFilterParams: radius is 2 (got {self.radius})")
        if len(self.wt) != 2 or any(not 0 <= v <= WEIGHT_MAX for v in self.wt):
            raise ValueError(f"TemporalFilterParams: wt is 2 weights in 0 .. {WEIGHT_MAX} (got {self.wt})")
        for name, lut in (("lut_b", self.lut_b), ("lut_p", self.lut_p)):
            if len(lut) != LUT_SIZE or any(not 0 <= v <= WEIGHT_MAX for v in lut):
                raise ValueError(f"TemporalFilterParams: {name} is {LUT_SIZE} entries in 0 .. {WEIGHT_MAX}")


def _check_format(fmt, H: int, W: int, what: str):
    if fmt.layout == "rgb24":
        raise ValueError(f"{what}: rgb24 frames hold no luma plane; the filter works on Y'CbCr codes")
    if fmt.depth not in (8, 10, 12, 16):
        raise ValueError(f"{what}: depth must be 8, 10, 12 or 16 (got {fmt.depth})")
    if H < 8 or W < 8:
        raise ValueError(f"{what}: image size must be at least 8 x 8 (got {H} x {W})")


def check_q(q, what: str = "temporal_filter") -> tuple:
    """``q`` as three ints in 1 .. 65535 (one number: the same for every plane)."""
    try:
        q = tuple(int(v) for v in q)
    except TypeError:
        q = (int(q),) * 3
    if len(q) != 3 or any(not 1 <= v <= Q_MAX for v in q):
        raise ValueError(f"{what}: q is one strength per plane, each 1 .. {Q_MAX} sixteenths of a code (got {q})")
    return q


def q_of_sigma(sigma, gain: float = 1.0) -> tuple:
    """``clamp(round(16 gain sigma), 1, 65535)`` per plane."""
    return tuple(min(max(int(round(16.0 * float(gain) * float(s))), 1), Q_MAX) for s in sigma)


# ----------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------
def temporal_filter(frames_u8, H: int, W: int, fmt: FrameFormat, flows, q, params: TemporalFilterParams | None = None, out=None,
                    first: int = 0):
    """The kernel alone.  ``frames_u8``: the resident clip, uint8 CUDA ``[T, >= frame_bytes]`` with contiguous rows (deep formats:
    little-endian 16-bit samples, even base and row stride).  ``flows``: float32 CUDA contiguous ``[n, 4, 2, H, W]``, slot j of row k the
    flow from frame ``first + k`` to frame ``first + k + OFFSETS[j]``; slots of neighbours that do not exist are never read.  ``q``: three
    strengths (or one for all planes).  Returns ``out`` (given, or new ``[n, frame_bytes]``): the filtered frames ``first .. first + n - 1``;
    it may not overlap the clip, and bytes of its rows beyond the frame are left alone.  One launch per 16 targets on the current
    stream; nothing synchronises."""
    import ctypes as C

    import torch

    from .metrics import _frame_rows
    H, W = int(H), int(W)
    _check_format(fmt, H, W, "temporal_filter")
    q = check_q(q)
    params = params or TemporalFilterParams()
    nbytes = frame_bytes(H, W, fmt)
    a, T, stride = _frame_rows(frames_u8, nbytes, fmt, "temporal_filter")
    if not isinstance(flows, torch.Tensor) or not flows.is_cuda or flows.dtype != torch.float32 or not flows.is_contiguous() \
            or flows.dim() != 5 or tuple(flows.shape[1:]) != (4, 2, H, W) or flows.device != a.device:
        raise ValueError(f"temporal_filter: flows must be contiguous float32 [n, 4, 2, {H}, {W}] on the frames' device (got "
                         f"{getattr(flows, 'dtype', type(flows).__name__)} {tuple(getattr(flows, 'shape', ()))})")
    n, first = int(flows.shape[0]), int(first)
    if n < 1 or first < 0 or first + n > T:
        raise ValueError(f"temporal_filter: targets {first} .. {first + n - 1} lie outside the {T} frames")
    if out is None:
        out = torch.empty((n, nbytes), dtype=torch.uint8, device=a.device)
    o, no, ostride = _frame_rows(out, nbytes, fmt, "temporal_filter")
    if no != n or o.device != a.device:
        raise ValueError(f"temporal_filter: out must hold {n} frames on the frames' device (got {no})")
    qc, wc = (C.c_uint32 * 3)(*q), (C.c_uint32 * 2)(*params.wt)
    lb, lp = (C.c_uint16 * LUT_SIZE)(*params.lut_b), (C.c_uint16 * LUT_SIZE)(*params.lut_p)
    L = _lib.lib()
    per_target = 8 * H * W * 4
    with torch.cuda.device(a.device):
        stream = _lib.current_stream(a.device)
        for i in range(0, n, MAX_BATCH):
            m = min(MAX_BATCH, n - i)
            _lib.check(L.gsvc_tfilter_frames(a.data_ptr(), stride, T, first + i, m, H, W, LAYOUTS[fmt.layout], fmt.depth,
                                             flows.data_ptr() + i * per_target, qc, wc, lb, lp, o.data_ptr() + i * ostride, ostride, stream),
                       "gsvc_tfilter_frames")
    return out


def noise_sums(frames_u8, H: int, W: int, fmt: FrameFormat):
    """The noise sums ``S`` of every frame and plane of a buffer of frames (what ``temporal_filter`` accepts) -> int64 ``[n, 3]`` on their
    device, exact.  One launch per 16 frames on the current stream; nothing synchronises."""
    import torch

    from .metrics import _frame_rows
    H, W = int(H), int(W)
    _check_format(fmt, H, W, "noise_sums")
    a, n, stride = _frame_rows(frames_u8, frame_bytes(H, W, fmt), fmt, "noise_sums")
    out = torch.empty((n, 3), dtype=torch.int64, device=a.device)
    L = _lib.lib()
    with torch.cuda.device(a.device):
        stream = _lib.current_stream(a.device)
        for i in range(0, n, MAX_BATCH):
            m = min(MAX_BATCH, n - i)
            _lib.check(L.gsvc_noise_sums(a.data_ptr() + i * stride, stride, m, H, W, LAYOUTS[fmt.layout], fmt.depth,
                                         out.data_ptr() + i * 24, stream), "gsvc_noise_sums")
    return out


def interior_samples(H: int, W: int, fmt: FrameFormat) -> tuple:
    """The samples of each plane that have all eight neighbours."""
    ch, cw = (H // 2, W // 2) if fmt.layout == "yuv420p" else (H, W)
    return ((H - 2) * (W - 2), (ch - 2) * (cw - 2), (ch - 2) * (cw - 2))


def noise_strength(sums, H: int, W: int, fmt: FrameFormat, gain: float = 1.0):
    """``(sigma, q)`` from ``noise_sums`` rows ``[n, 3]`` (a tensor, an array or nested lists): per plane ``sigma = sqrt(pi / 2) sum S /
    (6 n interior samples)`` in codes of the format's depth, pooled over the n frames, and ``q = clamp(round(16 gain sigma), 1, 65535)``.
    The estimator reads texture as noise, so this is a starting value."""
    if hasattr(sums, "detach"):
        sums = sums.detach().cpu().numpy()
    rows = np.asarray(sums, dtype=object).reshape(-1, 3)
    _check_format(fmt, int(H), int(W), "noise_strength")
    inner = interior_samples(int(H), int(W), fmt)
    sigma = tuple(math.sqrt(math.pi / 2.0) * float(sum(int(v) for v in rows[:, p])) / (6.0 * len(rows) * inner[p]) for p in range(3))
    return sigma, q_of_sigma(sigma, gain)


def code_lumas(frames_u8, H: int, W: int, fmt: FrameFormat):
    """The luma codes of a buffer of frames divided by ``2^depth - 1``: float32 contiguous ``[T, H, W]``, what ``flow.estimate_flow`` is
    given.  Plain tensor expressions; not a hot path."""
    import torch

    from .metrics import _frame_rows
    H, W = int(H), int(W)
    _check_format(fmt, H, W, "code_lumas")
    a, n, _ = _frame_rows(frames_u8, frame_bytes(H, W, fmt), fmt, "code_lumas")
    if fmt.depth > 8:
        y = a[:, :2 * H * W].contiguous().view(torch.int16).to(torch.int32).bitwise_and(0xFFFF)
    else:
        y = a[:, :H * W]
    return (y.to(torch.float32) / float((1 << fmt.depth) - 1)).reshape(n, H, W).contiguous()


def neighbour_flows(lumas, first: int, n: int, flow_params=None):
    """The ``[n, 4, 2, H, W]`` flows of the targets ``first .. first + n - 1`` of a clip's ``lumas`` (float32 CUDA ``[T, H, W]``): every
    pair ``(t, t + d)`` that exists goes through ``flow.estimate_flow`` in one batched call (a pair's result does not depend on the
    batch); slots without a neighbour are zero and never read.  8 bytes per pixel, neighbour and target frame."""
    import torch

    from .flow import FlowParams, estimate_flow
    T, H, W = (int(v) for v in lumas.shape)
    first, n = int(first), int(n)
    if n < 1 or first < 0 or first + n > T:
        raise ValueError(f"neighbour_flows: targets {first} .. {first + n - 1} lie outside the {T} frames")
    slots, src, dst = [], [], []
    for k in range(n):
        for j, d in enumerate(OFFSETS):
            if 0 <= first + k + d < T:
                slots.append(4 * k + j)
                src.append(first + k)
                dst.append(first + k + d)
    out = torch.zeros((n, 4, 2, H, W), dtype=torch.float32, device=lumas.device)
    if slots:
        index = lambda v: torch.tensor(v, dtype=torch.long, device=lumas.device)          # noqa: E731
        found = estimate_flow(lumas[index(src)].unsqueeze(1), lumas[index(dst)].unsqueeze(1), params=flow_params or FlowParams())
        out.view(4 * n, 2, H, W)[index(slots)] = found
    return out


def denoise_frames(frames_u8, H: int, W: int, fmt: FrameFormat, sigma="auto", gain: float = 1.0, flow_params=None, chunk: int = 8,
                   params: TemporalFilterParams | None = None):
    """The whole prefilter for one resident GOP: ``(denoised, log)``.  ``frames_u8``: uint8 CUDA ``[T, >= frame_bytes]`` (what
    ``temporal_filter`` accepts); ``denoised``: new ``[T, frame_bytes]`` on the same device.  ``sigma``: "auto" (``noise_sums`` and
    ``noise_strength`` over the GOP's own frames), one number for all planes, or ``(y, u, v)``, in codes of the format's depth;
    ``q = clamp(round(16 gain sigma), 1, 65535)``.  The flows come from ``neighbour_flows`` on ``code_lumas``, ``chunk`` target frames at a
    time.  ``log``: {"sigma", "q", "source": "auto" or "given", "gain", "psnr_y": the PSNR-Y of the output against the input over
    the GOP (``metrics.plane_sse``; inf when nothing changed)}.  A GOP of one frame has no neighbour and returns its input.

    Memory: the flows are 8 bytes per pixel, neighbour and target frame: 0.53 GB per chunk of 8 at 1080p, beside the estimator's own
    workspace."""
    import torch

    from .metrics import _frame_rows, plane_sse, psnr_of_sse
    H, W = int(H), int(W)
    _check_format(fmt, H, W, "denoise_frames")
    nbytes = frame_bytes(H, W, fmt)
    if isinstance(sigma, str):
        if sigma != "auto":
            raise ValueError(f"denoise_frames: sigma is 'auto', a number or (y, u, v) (got {sigma!r})")
        sig = None
    else:
        try:
            sig = tuple(float(v) for v in sigma)
        except TypeError:
            sig = (float(sigma),) * 3
        if len(sig) != 3 or any(not (v > 0.0 and math.isfinite(v)) for v in sig):
            raise ValueError(f"denoise_frames: sigma is 'auto', a positive number or three of them (got {sigma!r})")
    a, T, _ = _frame_rows(frames_u8, nbytes, fmt, "denoise_frames")
    if sig is None:
        (sig, q), source = noise_strength(noise_sums(a, H, W, fmt), H, W, fmt, gain), "auto"
    else:
        q, source = q_of_sigma(sig, gain), "given"
    chunk = max(int(chunk), 1)
    out = torch.empty((T, nbytes), dtype=torch.uint8, device=a.device)
    lumas = code_lumas(a, H, W, fmt)
    for i in range(0, T, chunk):
        m = min(chunk, T - i)
        flows = neighbour_flows(lumas, i, m, flow_params)
        temporal_filter(a, H, W, fmt, flows, q, params, out=out[i:i + m], first=i)
        del flows
    sse_y = int(plane_sse(out, a, H, W, fmt)[:, 0].sum().item())
    psnr = float(psnr_of_sse(torch.tensor(sse_y), T * H * W, float((1 << fmt.depth) - 1)).item())
    return out, {"sigma": [float(v) for v in sig], "q": [int(v) for v in q], "source": source, "gain": float(gain), "psnr_y": psnr}


def denoise_range(frames_host, H: int, W: int, fmt: FrameFormat, device, **kw):
    """``denoise_frames`` of a host array ``[T, frame_bytes]`` (one GOP of ``frames_in.open_video``) -> ``(uint8 numpy [T, frame_bytes],
    log)``: uploaded, filtered, downloaded."""
    import torch
    dev = torch.device(device)
    with torch.cuda.device(dev):
        up = torch.from_numpy(np.ascontiguousarray(frames_host)).to(dev)
        out, log = denoise_frames(up, H, W, fmt, **kw)
        return out.cpu().numpy(), log


def denoise_video(src, dst, sigma="auto", gain: float = 1.0, W: int | None = None, H: int | None = None, fmt: FrameFormat | None = None,
                  frame_ranges=None, device="cuda", flow_params=None, chunk: int = 8, params: TemporalFilterParams | None = None) -> dict:
    """File to file: the frames of ``src`` (``frames_in.open_video``) filtered and written to ``dst`` (``frames_out.open_sink``) in the
    source's own format.  ``frame_ranges``: a list of ``(first, stop)`` that tile the file (the GOPs of ``scene.plan_gops``); each range
    is filtered on its own, so nothing crosses a cut.  None: the whole file is one range.  Returns {"W", "H", "frames", "format",
    "ranges": [{"first", "stop", and the log of ``denoise_frames``}]}."""
    from .frames_in import open_video
    from .frames_out import open_sink
    hdr, frames = open_video(src, W, H, fmt)
    used = hdr["fmt"]
    Wf, Hf, T = int(hdr["W"]), int(hdr["H"]), int(frames.shape[0])
    _check_format(used, Hf, Wf, "denoise_video")
    ranges = [(0, T)] if frame_ranges is None else [(int(a), int(b)) for a, b in frame_ranges]
    at = 0
    for a, b in ranges:
        if a != at or b <= a or b > T:
            raise ValueError(f"denoise_video: frame_ranges must tile the {T} frames in order (got {ranges})")
        at = b
    if at != T:
        raise ValueError(f"denoise_video: frame_ranges must tile the {T} frames in order (got {ranges})")
    sink, _ = open_sink(dst, Wf, Hf, hdr.get("fps") or (30, 1), used)
    logs = []
    with sink:
        for a, b in ranges:
            out, log = denoise_range(frames[a:b], Hf, Wf, used, device, sigma=sigma, gain=gain, flow_params=flow_params, chunk=chunk,
                                     params=params)
            for row in out:
                sink.write(row)
            logs.append(dict(first=a, stop=b, **log))
    return {"W": Wf, "H": Hf, "frames": T, "format": used.name, "ranges": logs}


def parse_sigma(text):
    """The ``type=`` of an ``{auto,SIGMA}`` command-line option (``--denoise`` of tools/gsvc_encode.py and tools/fit_synthetic.py,
    ``--sigma`` of tools/denoise_video.py): "auto", or a positive finite number of codes as a float; anything else is an
    ``argparse.ArgumentTypeError``, which argparse reports under the option's own name."""
    import argparse
    if text is None or text == "auto":
        return text
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not (v > 0.0 and math.isfinite(v)):
        raise argparse.ArgumentTypeError(f"'auto' or a positive noise sigma in codes is expected (got {text!r})")
    return v
