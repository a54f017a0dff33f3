"""Film grain: estimated at the encoder, synthesised on the decoder's device (host side of csrc/grain.hip).

A Gaussian-splat model at 0.06 - 0.10 bpp cannot represent sensor noise or film grain: the fit delivers flat regions as flat.  As AV1's
film-grain tool and the grain SEI of HEVC / VVC do, the encoder measures the grain it removed (``grain_stats`` on the source's codes
against the decoder's own, ``fit_grain``), ships a ``GrainParams`` (122 bytes, the optional section GRAN of a bitstream file) and the
decoder adds statistically equal grain to the delivered samples, outside the coding loop (``apply_grain``).  The picture hashes (PHSH)
stay those of the UNGRAINED picture; grain is a deterministic post-process of it.

Synthesis, exactly
------------------
Everything is an integer; ``>>`` is the arithmetic shift (floor).  ``GOLD = 0x9E3779B97F4A7C15``; 64-bit products and sums wrap.

    mix(z):   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;   z = (z ^ z >> 27) * 0x94D049BB133111EB;   z ^ z >> 31          (splitmix64)

White noise.  For the GLOBAL frame index ``f`` (the frame's index in the whole clip, 0 .. 2^32 - 1), the plane ``p`` (0 Y, 1 U, 2 V) and
the sample ``(y, x)`` of the plane's own grid — also outside the picture, y and x from -1:

    key(f, p) = mix(seed + (3 f + p + 1) GOLD)
    h         = mix(key(f, p) + (((y + 1) << 32) | ((x + 1) >> 1)) GOLD)
    w         = h >> 32 if (x + 1) is odd, else h & 0xFFFFFFFF              (one hash serves two horizontally adjacent samples)
    g(y, x)   = (the sum of the four bytes of w) - 510

an Irwin-Hall integer in -510 .. 510 with mean 0 and variance 4 (256^2 - 1) / 12 = 21845.  It depends on (seed, f, p, y, x) alone: not
on tiles, batches or launches.

Correlation.  A separable 3-tap filter in Q6, ``[kx, 64, kx]`` along a row and ``[ky, 64, ky]`` down a column, over g including the
positions outside the picture (edges have no special case), and ONE rounding shift:

    t(y, x) = kx[p] (g(y, x - 1) + g(y, x + 1)) + 64 g(y, x)
    n(y, x) = (ky[p] (t(y - 1, x) + t(y + 1, x)) + 64 t(y, x) + 2048) >> 12

``n`` has variance 21845 (4096 + 2 kx^2) (4096 + 2 ky^2) / 2^24 (``noise_variance``) and lag-1 correlations 128 k / (4096 + 2 k^2)
along the axis of tap k (``lag1``; 0.444 at k = 16, 0.667 at k = 32), lag-2 correlations k^2 / (4096 + 2 k^2).

Strength.  With ``c`` the sample's ungrained code and ``m`` the co-located UNGRAINED luma code (the luma plane: c itself; 4:4:4 chroma:
the luma code at (y, x); 4:2:0 chroma: ``(a + b + c + d + 2) >> 2`` of the luma codes at (2y, 2x), (2y, 2x + 1), (2y + 1, 2x),
(2y + 1, 2x + 1)):

    l = min(m >> (depth - 8), 255);    i = l >> 4;    r = l & 15
    s = (scale[p][i] (16 - r) + scale[p][i + 1] r + 8) >> 4

``scale[p]`` are 17 uint16 strengths at 8-bit-normalised luma 0, 16, .., 256, piecewise linear in between.  Their Q format: a strength is
a Q16 multiplier of ``n`` in units of an 8-bit code — the grain of an 8-bit sample is n s / 2^16 codes, so a flat strength s gives grain
of standard deviation ``sqrt(noise_variance(kx, ky)) s / 2^16`` 8-bit codes (s = 443 is about one code for white noise; 65535 is about
148).  A deeper format multiplies by 2^(depth - 8):

    grain = (n s + 2^(S - 1)) >> S,    S = 24 - depth
    out   = min(max(c + grain, min(lo, c)), max(hi, c))

``lo .. hi`` is the format's nominal range: 16 .. 235 (luma) and 16 .. 240 (chroma) times 2^(depth - 8) for ``limited``, 0 .. 2^depth - 1
for ``full``.  Grain never moves a sample out of the nominal range, and a sample whose grain is 0 keeps its code whatever it was: an
all-zero ``scale`` returns the input bytes unchanged.  Layouts ``yuv420p`` and ``yuv444p`` at depths 8, 10, 12 and 16; ``rgb24`` raises
``ValueError`` (grain lives in the delivered Y'CbCr domain).

Statistics, exactly
-------------------
``grain_stats(src, dec)`` -> int64 ``[3, 16, 6]``: exact 64-bit integer sums, independent of the order of summation.  Every plane is cut
into whole 8 x 8 blocks of its own sample grid; partial blocks at the right and bottom edges are skipped.  Per block, with ``up =
2^(depth - 8)``:

    r    = src - dec                                               (64 code differences)
    A    = the sum of the 56 + 56 absolute differences of horizontally and vertically adjacent DEC codes inside the block
    bin  = min((the sum of the dec LUMA codes of the co-located region >> q) >> (depth - 8), 255) >> 4
           (the region is the block itself, q = 6, for luma and 4:4:4 chroma, and the 16 x 16 luma codes under it, q = 8, for 4:2:0 chroma)

A block counts when ``A <= flat_threshold up`` and every ``|r| <= max_residual up`` (a larger residual is fit error, not grain, and the
bound keeps every sum inside int64).  Each counting block adds to row ``[plane][bin]``:

    1,   S1 = sum r,   S2 = sum r^2,   S1^2,   Px = sum r(y, x) r(y, x + 1) over the 56 pairs,   Py = sum r(y, x) r(y + 1, x) likewise

``fit_grain`` (host, float64, on the summed rows) is described at the function.  ``DEFAULT_FLAT_THRESHOLD`` and ``DEFAULT_MIN_BLOCKS``
are starting values nobody has measured on real content.

Importing this module needs neither a GPU nor the built library; ``apply_grain`` and ``grain_stats`` do (no CPU fallback).
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass

import numpy as np

from . import _lib
from .frames_out import LAYOUTS, MATRICES, MAX_BATCH, RANGES, ROUNDINGS, FrameFormat, frame_bytes

GRAIN_VERSION = 1
KNOTS = 17                          # strengths per plane, at 8-bit-normalised luma 0, 16, .., 256
BINS = 16                           # luma bins of the statistics
TAP_MAX = 32
NOISE_VAR = 21845                   # of g: 4 (256^2 - 1) / 12
SCALE_ONE = 1 << 16                 # the Q16 of a strength
DEFAULT_FLAT_THRESHOLD = 224        # A of a block in 8-bit codes: a mean neighbour difference of 2.  A starting value, not measured
DEFAULT_MAX_RESIDUAL = 32           # |src - dec| in 8-bit codes above which a block is fit error, not grain
DEFAULT_MIN_BLOCKS = 16             # blocks a luma bin needs before its variance is believed.  A starting value, not measured
_LAYOUT_NAMES = {v: k for k, v in LAYOUTS.items()}
_MATRIX_NAMES = {v: k for k, v in MATRICES.items()}
_RANGE_NAMES = {v: k for k, v in RANGES.items()}
_ROUNDING_NAMES = {v: k for k, v in ROUNDINGS.items()}
_PACK = struct.Struct("<BQBBBBB51H3b3b")          # version, seed, source (layout, depth, matrix, range, rounding), scale, kx, ky


def noise_variance(kx: int, ky: int) -> float:
    """The variance of the filtered noise ``n``."""
    return NOISE_VAR * (4096 + 2 * kx * kx) * (4096 + 2 * ky * ky) / float(1 << 24)


def lag1(k: int) -> float:
    """The lag-1 correlation of ``n`` along the axis whose tap is ``k``."""
    return 128.0 * k / (4096 + 2 * k * k)


def lag2(k: int) -> float:
    return float(k * k) / (4096 + 2 * k * k)


@dataclass(frozen=True)
class GrainParams:
    """Everything the synthesis needs, integers only (the module's docstring says what each does): ``seed`` (64 bits), ``scale`` (per
    plane 17 uint16 strengths), ``kx`` / ``ky`` (per plane one tap each way, -32 .. 32) and ``source``, the ``FrameFormat`` the statistics
    were taken in.  ``source`` is RECORDED, not used for rescaling: a decode into another range or depth applies the strengths as they
    are (per 8-bit code of the format decoded to)."""
    seed: int
    scale: tuple
    kx: tuple = (0, 0, 0)
    ky: tuple = (0, 0, 0)
    source: FrameFormat = FrameFormat("yuv420p")

    def __post_init__(self):
        object.__setattr__(self, "seed", int(self.seed))
        object.__setattr__(self, "scale", tuple(tuple(int(v) for v in row) for row in self.scale))
        object.__setattr__(self, "kx", tuple(int(v) for v in self.kx))
        object.__setattr__(self, "ky", tuple(int(v) for v in self.ky))
        if not 0 <= self.seed < 1 << 64:
            raise ValueError(f"GrainParams: seed must be 0 .. 2^64 - 1 (got {self.seed})")
        if len(self.scale) != 3 or any(len(row) != KNOTS for row in self.scale):
            raise ValueError(f"GrainParams: scale is 3 planes of {KNOTS} strengths")
        if any(not 0 <= v <= 65535 for row in self.scale for v in row):
            raise ValueError("GrainParams: a strength must be 0 .. 65535")
        for name, taps in (("kx", self.kx), ("ky", self.ky)):
            if len(taps) != 3 or any(not -TAP_MAX <= v <= TAP_MAX for v in taps):
                raise ValueError(f"GrainParams: {name} is 3 taps in -{TAP_MAX} .. {TAP_MAX} (got {taps})")
        if not isinstance(self.source, FrameFormat) or self.source.layout == "rgb24":
            raise ValueError("GrainParams: source must be a yuv420p / yuv444p FrameFormat")

    @property
    def is_zero(self) -> bool:
        return not any(v for row in self.scale for v in row)

    def pack(self) -> bytes:
        """122 bytes, little-endian: uint8 version (1) | uint64 seed | uint8 layout, depth, matrix, range, rounding of ``source`` (the enums
        of include/gsvc_hip.h) | uint16 scale[3][17] | int8 kx[3] | int8 ky[3]."""
        s = self.source
        return _PACK.pack(GRAIN_VERSION, self.seed, LAYOUTS[s.layout], s.depth, MATRICES[s.matrix], RANGES[s.range], ROUNDINGS[s.rounding_used],
                          *[v for row in self.scale for v in row], *self.kx, *self.ky)

    @classmethod
    def unpack(cls, payload: bytes) -> "GrainParams":
        """The inverse of ``pack``; every length and range error is a ``BitstreamError("GRAN", ...)``."""
        from .bitstream import BitstreamError
        payload = bytes(payload)
        if len(payload) < 1:
            raise BitstreamError("GRAN", "truncated: the section is empty")
        if payload[0] != GRAIN_VERSION:
            raise BitstreamError("GRAN", f"grain version {payload[0]} is not readable by this decoder (it reads {GRAIN_VERSION})")
        if len(payload) != _PACK.size:
            raise BitstreamError("GRAN", f"{'truncated' if len(payload) < _PACK.size else 'too long'}: {_PACK.size} bytes expected, {len(payload)} present")
        f = _PACK.unpack(payload)
        layout, depth, matrix, rng, rounding = f[2:7]
        try:
            source = FrameFormat(_LAYOUT_NAMES[layout], _MATRIX_NAMES[matrix], _RANGE_NAMES[rng], _ROUNDING_NAMES[rounding], depth)
            return cls(seed=f[1], scale=(f[7:24], f[24:41], f[41:58]), kx=f[58:61], ky=f[61:64], source=source)
        except (KeyError, ValueError) as e:
            raise BitstreamError("GRAN", f"a field is out of range ({e})") from e

    def as_c(self):
        c = _lib.GrainParamsC()
        c.seed = self.seed
        for p in range(3):
            for i in range(KNOTS):
                c.scale[p][i] = self.scale[p][i]
            c.kx[p], c.ky[p] = self.kx[p], self.ky[p]
        return c

    def summary(self) -> dict:
        """What an encoder's log says of the parameters."""
        return {"seed": self.seed, "scale": [list(row) for row in self.scale], "kx": list(self.kx), "ky": list(self.ky),
                "source": self.source.name}


# ----------------------------------------------------------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------------------------------------------------------
def _check_format(fmt, what: str):
    if fmt.layout == "rgb24":
        raise ValueError(f"{what}: rgb24 frames hold no luma plane; grain lives in the delivered Y'CbCr domain")


def apply_grain(frames_u8, H: int, W: int, fmt: FrameFormat, params: GrainParams, first_frame: int = 0, frame_ids=None):
    """Add the grain of ``params`` IN PLACE to a buffer of delivered frames: uint8 CUDA ``[n, >= frame_bytes]`` with contiguous rows (or
    one flat frame; deep formats: little-endian 16-bit samples, even base and row stride).  Bytes of a row beyond the frame are left
    alone.  Row k is frame ``first_frame + k`` of the clip, or ``frame_ids[k]``: a frame's grain is a function of that index, not of
    the batch it travels in.  One launch per 16 frames on the current stream; nothing synchronises.  Returns ``frames_u8``."""
    import ctypes as C

    import torch

    from .metrics import _frame_rows
    H, W = int(H), int(W)
    _check_format(fmt, "apply_grain")
    a, n, stride = _frame_rows(frames_u8, frame_bytes(H, W, fmt), fmt, "apply_grain")
    ids = [int(first_frame) + k for k in range(n)] if frame_ids is None else [int(v) for v in frame_ids]
    if len(ids) != n:
        raise ValueError(f"apply_grain: {len(ids)} frame ids for {n} frames")
    if any(not 0 <= v < 1 << 32 for v in ids):
        raise ValueError("apply_grain: a frame index must be 0 .. 2^32 - 1")
    if params.is_zero:
        return frames_u8
    c = params.as_c()
    L = _lib.lib()
    with torch.cuda.device(a.device):
        stream = _lib.current_stream(a.device)
        for i in range(0, n, MAX_BATCH):
            m = min(MAX_BATCH, n - i)
            _lib.check(L.gsvc_grain_apply(a.data_ptr() + i * stride, stride, m, H, W, LAYOUTS[fmt.layout], fmt.depth, RANGES[fmt.range],
                                          C.byref(c), (C.c_int64 * m)(*ids[i:i + m]), stream), "gsvc_grain_apply")
    return frames_u8


def grain_stats(src_u8, dec_u8, H: int, W: int, fmt: FrameFormat, flat_threshold: int = DEFAULT_FLAT_THRESHOLD,
                max_residual: int = DEFAULT_MAX_RESIDUAL):
    """The flat-block statistics of the source's codes against the decoder's (two buffers of ``fmt`` frames, what ``plane_sse`` accepts)
    -> int64 ``[3, 16, 6]`` on their device, summed over the frames: per plane and luma bin (blocks, S1, S2, S1^2, Px, Py) as the
    module's docstring defines them.  Exact integer sums: bit-identical run to run.  One launch and a memset on the current stream;
    nothing synchronises."""
    import torch

    from .metrics import _frame_rows
    H, W = int(H), int(W)
    _check_format(fmt, "grain_stats")
    nbytes = frame_bytes(H, W, fmt)
    a, n, sa = _frame_rows(src_u8, nbytes, fmt, "grain_stats")
    b, nb, sb = _frame_rows(dec_u8, nbytes, fmt, "grain_stats")
    if nb != n or a.device != b.device:
        raise ValueError(f"grain_stats: the two buffers must hold the same number of frames on one device (got {n} and {nb})")
    out = torch.empty((3, BINS, 6), dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().gsvc_grain_stats(a.data_ptr(), sa, b.data_ptr(), sb, n, H, W, LAYOUTS[fmt.layout], fmt.depth,
                                               int(flat_threshold), int(max_residual), out.data_ptr(), _lib.current_stream(a.device)),
                   "gsvc_grain_stats")
    return out


# ----------------------------------------------------------------------------------------------------------------------------
# the fit (host)
# ----------------------------------------------------------------------------------------------------------------------------
def _dc_share(kx: int, ky: int) -> float:
    """E[S1^2 / 64] / (64 sigma^2) of an 8 x 8 block of the filtered noise: what removing the block's mean takes from the variance."""
    mx = 1.0 + (14.0 * lag1(kx) + 12.0 * lag2(kx)) / 8.0
    my = 1.0 + (14.0 * lag1(ky) + 12.0 * lag2(ky)) / 8.0
    return mx * my / 64.0


def _rows_as_ints(stats):
    """``[3, 16, 6]`` statistics (a tensor, an array or nested lists of ints) as nested lists of Python ints."""
    if hasattr(stats, "detach"):
        stats = stats.detach().cpu().numpy()
    a = np.asarray(stats, dtype=object)
    if a.shape != (3, BINS, 6):
        raise ValueError(f"fit_grain: statistics are [3, {BINS}, 6] (got {a.shape})")
    return [[[int(v) for v in row] for row in plane] for plane in a]


def fit_grain(stats, seed: int, gain: float = 1.0, min_blocks: int = DEFAULT_MIN_BLOCKS, source: FrameFormat = FrameFormat("yuv420p")):
    """``GrainParams`` from summed ``grain_stats`` rows, in float64 on the host.  ``source``: the format the statistics were taken in
    (its depth scales the variances to 8-bit codes; it is recorded in the result).  Per plane:

      taps       over the bins with at least ``min_blocks`` blocks, the pooled block-DC-removed moments
                 V = (sum S2 - sum S1^2 / 64) / (64 N),  Cx = (sum Px - 56 sum S1^2 / 4096) / (56 N),  Cy likewise, give the measured
                 lag-1 correlations Cx / V and Cy / V.  For taps (kx, ky) the same moments of the model's noise are predicted — removing
                 the mean of an 8 x 8 block takes the share e = ``_dc_share(kx, ky)`` of the variance, so the prediction is
                 (lag1(k) - e) / (1 - e) —, and the (kx, ky) in -32 .. 32 whose two predictions are nearest (least squares) is taken.
      strengths  per such bin sigma^2 = max(V_bin / (1 - e) - 1 / 12, 0) in squared source codes (1 / 12: the rounding of the source's
                 grain to whole codes, which the synthesis repeats), sigma_8 = sigma / 2^(depth - 8), and the bin's strength is
                 gain sigma_8 2^16 / sqrt(noise_variance(kx, ky)).  Bins with fewer blocks take theirs from the nearest populated bins
                 (linear between two, the nearest one's beyond the ends).  Knot i (luma 16 i) is the mean of bins i - 1 and i (knots 0
                 and 16: the bin beside them), rounded and clamped to 65535.  A plane without a populated bin gets zero strength and
                 zero taps."""
    rows = _rows_as_ints(stats)
    up = float(1 << (source.depth - 8))
    scale, kxs, kys = [], [], []
    for p in range(3):
        ok = [b for b in range(BINS) if rows[p][b][0] >= max(int(min_blocks), 1)]
        if not ok:
            scale.append((0,) * KNOTS)
            kxs.append(0)
            kys.append(0)
            continue
        N = sum(rows[p][b][0] for b in ok)
        S2, Q, Px, Py = (sum(rows[p][b][j] for b in ok) for j in (2, 3, 4, 5))
        V = (S2 - Q / 64.0) / (64.0 * N)
        kx = ky = 0
        if V > 0:
            rx, ry = (Px - 56.0 * Q / 4096.0) / (56.0 * N) / V, (Py - 56.0 * Q / 4096.0) / (56.0 * N) / V
            best = None
            for cx in range(-TAP_MAX, TAP_MAX + 1):
                for cy in range(-TAP_MAX, TAP_MAX + 1):
                    e = _dc_share(cx, cy)
                    d = ((lag1(cx) - e) / (1.0 - e) - rx) ** 2 + ((lag1(cy) - e) / (1.0 - e) - ry) ** 2
                    if best is None or d < best[0]:
                        best = (d, cx, cy)
            _, kx, ky = best
        e = _dc_share(kx, ky)
        unit = math.sqrt(noise_variance(kx, ky))
        per_bin = {}
        for b in ok:
            n_b, _, s2, q = rows[p][b][:4]
            var = max((s2 - q / 64.0) / (64.0 * n_b) / (1.0 - e) - 1.0 / 12.0, 0.0)
            per_bin[b] = float(gain) * math.sqrt(var) / up * SCALE_ONE / unit
        full = []
        for b in range(BINS):
            if b in per_bin:
                full.append(per_bin[b])
                continue
            below, above = [c for c in ok if c < b], [c for c in ok if c > b]
            if below and above:
                lo, hi = below[-1], above[0]
                full.append(per_bin[lo] + (per_bin[hi] - per_bin[lo]) * (b - lo) / (hi - lo))
            else:
                full.append(per_bin[below[-1] if below else above[0]])
        knots = [full[0]] + [(full[i - 1] + full[i]) / 2.0 for i in range(1, BINS)] + [full[BINS - 1]]
        scale.append(tuple(min(int(round(v)), 65535) for v in knots))
        kxs.append(kx)
        kys.append(ky)
    return GrainParams(seed=int(seed) & 0xFFFFFFFFFFFFFFFF, scale=tuple(scale), kx=tuple(kxs), ky=tuple(kys), source=source)


def blocks_used(stats) -> list:
    """Per plane, the blocks that counted."""
    rows = _rows_as_ints(stats)
    return [sum(rows[p][b][0] for b in range(BINS)) for p in range(3)]
