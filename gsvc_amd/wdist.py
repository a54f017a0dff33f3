"""Spatially weighted distortion: the weight maps of a fit, and the weighted PSNR that measures what they bought.

A fit may weight its image terms per cell of ``cell`` x ``cell`` pixels (the cells of ``detail.map_shape``): a region of interest the user
names, an activity map of the clip (what x264 / x265 call AQ), a map from a file, or their product.  The maps only shape the fit
(``loss_utils.wssim_l1``, csrc/wdist.hip): nothing of them reaches the bitstream.

  ``normalise``         scale each frame's map so that its pixel-weighted mean is 1: the weighted terms stay on the scale of the plain
                        ones, and ``lambda_dssim`` / ``lmbda`` keep their meaning.
  ``activity_weights``  from the uint32 map of ``detail.cube_detail``: ``w = 2^(-strength (e - mean e))`` with ``e = log2(1 + a)`` and
                        ``a`` the detail per pixel in 8-bit code units.  ``strength > 0`` moves weight to flat cells (the AQ direction),
                        ``strength < 0`` to detail.
  ``roi_weights``       rectangles in pixels over a base of 1; a cell's weight is the mean over its own pixels.
  ``load_weights``      a ``.npy`` of ``[Hc, Wc]`` or ``[T, Hc, Wc]``.
  ``fit_weights``       what ``codec.new_fit`` builds from its arguments: the sources multiply before the one normalisation.
  ``block_sse``         exact per-cell luma SSE of two buffers of delivered frames (csrc/wdist.hip, gsvc_frames_block_sse).
  ``weighted_psnr_y``   ``10 log10(peak^2 H W / sum w sse)`` per frame and pooled, in float64.

The maps are tiny: everything here runs on the host in float64 and rounds once, to the float32 the kernels read.
``DEFAULT_STRENGTH`` and ``DEFAULT_CLAMP`` are starting values, not measured ones.
"""
from __future__ import annotations

import numpy as np

from .detail import CELLS, DEFAULT_CELL, map_shape

DEFAULT_STRENGTH = 0.5     # a starting value, not measured
DEFAULT_CLAMP = 4.0        # weights before normalisation stay within [1 / clamp, clamp]; a starting value, not measured
WEIGHTINGS = (None, "activity")


def check_cell(cell, what: str = "wdist"):
    if isinstance(cell, bool) or cell not in CELLS:
        raise ValueError(f"{what}: cell must be one of {', '.join(str(c) for c in CELLS)} (got {cell!r})")
    return int(cell)


def cell_pixels(H: int, W: int, cell: int) -> np.ndarray:
    """float64 ``[Hc, Wc]``: the pixels of each cell, the last row and column partial where ``cell`` does not divide the side."""
    Hc, Wc = map_shape(H, W, cell)
    rows = np.minimum(cell, int(H) - cell * np.arange(Hc)).astype(np.float64)
    cols = np.minimum(cell, int(W) - cell * np.arange(Wc)).astype(np.float64)
    return rows[:, None] * cols[None, :]


def _host64(maps, what: str) -> np.ndarray:
    if hasattr(maps, "detach"):
        maps = maps.detach().cpu().numpy()
    return np.asarray(maps, dtype=np.float64)


def _normalise64(maps, H: int, W: int, cell: int, what: str = "normalise") -> np.ndarray:
    cell = check_cell(cell, what)
    m = _host64(maps, what)
    Hc, Wc = map_shape(H, W, cell)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or m.shape[1:] != (Hc, Wc) or m.shape[0] < 1:
        raise ValueError(f"{what}: maps of a {int(H)} x {int(W)} picture at cell {cell} must be [T, {Hc}, {Wc}] (got {tuple(m.shape)})")
    if not np.isfinite(m).all():
        raise ValueError(f"{what}: weights must be finite")
    if (m < 0).any():
        raise ValueError(f"{what}: weights must not be negative")
    mass = (m * cell_pixels(H, W, cell)[None]).sum(axis=(1, 2))
    if (mass <= 0).any():
        raise ValueError(f"{what}: frame {int(np.argmax(mass <= 0))} has no weight at all (every cell is 0)")
    return m * (float(int(H) * int(W)) / mass)[:, None, None]


def _to_f32(m64: np.ndarray):
    import torch
    return torch.from_numpy(np.ascontiguousarray(m64.astype(np.float32)))


def normalise(maps, H: int, W: int, cell: int):
    """Each frame's map scaled so that its pixel-weighted mean is 1: ``sum_cells w n_pix(cell) = H W``, partial cells counting their own
    pixels -> float32 CPU tensor ``[T, Hc, Wc]``.  Refuses non-finite or negative weights and a frame whose weights are all 0."""
    return _to_f32(_normalise64(maps, H, W, cell))


def _activity64(dmap, H: int, W: int, cell: int, depth: int, strength: float, clamp: float) -> np.ndarray:
    cell = check_cell(cell, "activity_weights")
    strength, clamp, depth = float(strength), float(clamp), int(depth)
    if not np.isfinite(strength):
        raise ValueError(f"activity_weights: strength must be finite (got {strength!r})")
    if not (np.isfinite(clamp) and clamp >= 1.0):
        raise ValueError(f"activity_weights: clamp must be a number >= 1 (got {clamp!r})")
    if not 8 <= depth <= 16:
        raise ValueError(f"activity_weights: depth must be 8 .. 16 (got {depth})")
    if hasattr(dmap, "detach"):
        import torch
        if dmap.dtype == torch.uint32:          # (numpy has the type; torch cannot widen it itself)
            dmap = dmap.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    d = _host64(dmap, "activity_weights")
    Hc, Wc = map_shape(H, W, cell)
    if d.ndim != 3 or d.shape[1:] != (Hc, Wc) or d.shape[0] < 1:
        raise ValueError(f"activity_weights: the detail map must be [T, {Hc}, {Wc}] (got {tuple(d.shape)})")
    n_pix = cell_pixels(H, W, cell)[None]
    e = np.log2(1.0 + d / (n_pix * 2.0 ** (depth - 8)))
    mean_e = (e * n_pix).sum() / (d.shape[0] * float(int(H) * int(W)))
    return np.clip(2.0 ** (-strength * (e - mean_e)), 1.0 / clamp, clamp)


def activity_weights(dmap, H: int, W: int, cell: int, depth: int, strength: float = DEFAULT_STRENGTH, clamp: float = DEFAULT_CLAMP):
    """Activity-adaptive weights from the uint32 ``[T, Hc, Wc]`` map of ``detail.cube_detail`` (codes of ``depth`` bits):
    ``a = dmap / (n_pix 2^(depth - 8))`` is the detail per pixel in 8-bit code units, ``e = log2(1 + a)``, ``mean e`` its pixel-weighted
    mean over the WHOLE clip, ``w = 2^(-strength (e - mean e))`` clamped to ``[1 / clamp, clamp]`` and then normalised per frame ->
    float32 CPU tensor ``[T, Hc, Wc]``.  ``strength > 0`` moves weight to flat cells, ``strength < 0`` to detail, 0 gives all ones.
    Both defaults are starting values that nobody has measured."""
    return _to_f32(_normalise64(_activity64(dmap, H, W, cell, depth, strength, clamp), H, W, cell, "activity_weights"))


def _roi64(H: int, W: int, cell: int, rects, T: int) -> np.ndarray:
    cell = check_cell(cell, "roi_weights")
    H, W, T = int(H), int(W), int(T)
    if T < 1:
        raise ValueError(f"roi_weights: T must be positive (got {T})")
    pix = np.ones((H, W), dtype=np.float64)
    for r in rects:
        try:
            x, y, w, h, wt = r
            x, y, w, h, wt = int(x), int(y), int(w), int(h), float(wt)
        except (TypeError, ValueError):
            raise ValueError(f"roi_weights: a rectangle is (x, y, w, h, weight) (got {r!r})") from None
        if w <= 0 or h <= 0:
            raise ValueError(f"roi_weights: a rectangle needs a positive width and height (got {r!r})")
        if not np.isfinite(wt) or wt < 0:
            raise ValueError(f"roi_weights: a rectangle's weight must be finite and not negative (got {r!r})")
        pix[max(y, 0):max(min(y + h, H), 0), max(x, 0):max(min(x + w, W), 0)] = wt          # later rectangles override earlier ones
    Hc, Wc = map_shape(H, W, cell)
    padded = np.zeros((Hc * cell, Wc * cell), dtype=np.float64)
    padded[:H, :W] = pix
    cells = padded.reshape(Hc, cell, Wc, cell).sum(axis=(1, 3)) / cell_pixels(H, W, cell)
    return np.broadcast_to(cells[None], (T, Hc, Wc)).copy()


def roi_weights(H: int, W: int, cell: int, rects, T: int):
    """Region-of-interest weights: ``rects = [(x, y, w, h, weight), ...]`` in pixels over a base of 1, later rectangles overriding earlier
    ones (parts outside the picture are ignored); a cell's weight is the mean over its own pixels; then normalised -> float32 CPU tensor
    ``[T, Hc, Wc]``, every frame the same.  A weight of 0 ("don't care") is allowed, a picture that is 0 everywhere is not."""
    return _to_f32(_normalise64(_roi64(H, W, cell, rects, T), H, W, cell, "roi_weights"))


def _load64(path, T: int, H: int, W: int, cell: int) -> np.ndarray:
    cell = check_cell(cell, "load_weights")
    m = np.load(path, allow_pickle=False)
    Hc, Wc = map_shape(H, W, cell)
    if m.dtype.kind not in "fiu" or m.shape not in ((Hc, Wc), (int(T), Hc, Wc)):
        raise ValueError(f"load_weights: {path}: a numeric array of [{Hc}, {Wc}] or [{int(T)}, {Hc}, {Wc}] is needed for {int(T)} frames of "
                         f"{int(H)} x {int(W)} at cell {cell} (got {m.dtype} {tuple(m.shape)})")
    m = m.astype(np.float64)
    return np.broadcast_to(m[None], (int(T), Hc, Wc)).copy() if m.ndim == 2 else m


def load_weights(path, T: int, H: int, W: int, cell: int):
    """The weights of a ``.npy`` file, ``[Hc, Wc]`` (every frame) or ``[T, Hc, Wc]``, normalised -> float32 CPU tensor ``[T, Hc, Wc]``."""
    return _to_f32(_normalise64(_load64(path, T, H, W, cell), H, W, cell, "load_weights"))


def scale_rects(rects, src_hw, dst_hw):
    """Rectangles given in the pixels of a ``src_hw = (H, W)`` picture in those of ``dst_hw`` (reduced-resolution coding: the fit sees the
    coded size, the user speaks of the display): edges rounded to the nearest pixel, never thinner than one."""
    (sh, sw), (dh, dw) = src_hw, dst_hw
    if (int(sh), int(sw)) == (int(dh), int(dw)):
        return [tuple(r) for r in rects]
    out = []
    for x, y, w, h, wt in rects:
        x0, x1 = round(x * dw / sw), round((x + w) * dw / sw)
        y0, y1 = round(y * dh / sh), round((y + h) * dh / sh)
        out.append((int(x0), int(y0), max(int(x1 - x0), 1), max(int(y1 - y0), 1), wt))
    return out


def parse_roi(text: str):
    """``"X,Y,W,H:WEIGHT"`` of the command lines -> ``(x, y, w, h, weight)``."""
    try:
        box, wt = text.split(":")
        x, y, w, h = (int(v) for v in box.split(","))
        return x, y, w, h, float(wt)
    except ValueError:
        raise ValueError(f"--roi takes X,Y,W,H:WEIGHT (got {text!r})") from None


def fit_weights(cube, weighting=None, strength: float = DEFAULT_STRENGTH, cell: int | None = None, roi=None, weight_file=None,
                clamp: float = DEFAULT_CLAMP, roi_base_hw=None):
    """The weight maps of a fit on ``cube`` and what the log says of them -> ``(float32 CPU tensor [T, Hc, Wc], info)``, or
    ``(None, None)`` when nothing asks for weights.  The sources (the clip's activity, rectangles, a file) multiply in float64 and are
    normalised once.  The activity map is that of the cube's own frames (``detail.cube_detail``: a ``frame_range`` cube = one group of
    pictures, coded-size frames under reduced-resolution coding); rectangles are given in the pixels of ``roi_base_hw`` (None: the cube's
    own) and scaled to the cube's."""
    if weighting not in WEIGHTINGS:
        raise ValueError(f"weighting must be None or 'activity' (got {weighting!r})")
    roi = list(roi) if roi else []
    if weighting is None and not roi and weight_file is None:
        return None, None
    cell = check_cell(DEFAULT_CELL if cell is None else cell, "weighting")
    T, H, W = int(cube.len_z_frames), int(cube.height), int(cube.width)
    raw, sources = np.ones((T,) + map_shape(H, W, cell), dtype=np.float64), []
    info = {"cell": cell}
    if weighting == "activity":
        from .detail import cube_detail
        fmt = getattr(cube, "fmt", None)
        depth = int(fmt.depth) if (fmt is not None and fmt.layout != "rgb24" and hasattr(cube, "luma_detail")) else 16
        raw *= _activity64(cube_detail(cube, cell), H, W, cell, depth, strength, clamp)
        sources.append("activity")
        info.update(strength=float(strength), clamp=float(clamp))
    if roi:
        rects = scale_rects(roi, roi_base_hw or (H, W), (H, W))
        raw *= _roi64(H, W, cell, rects, T)
        sources.append("roi")
        info["roi"] = [list(r) for r in rects]
    if weight_file is not None:
        raw *= _load64(weight_file, T, H, W, cell)
        sources.append("file")
    maps = _to_f32(_normalise64(raw, H, W, cell, "weighting"))
    info.update(sources=sources, min=float(maps.min()), max=float(maps.max()))
    return maps, info


def block_sse(a_u8, b_u8, H: int, W: int, fmt, cell: int):
    """Sum of squared luma code differences per cell of two buffers of ``yuv420p`` / ``yuv444p`` frames (what ``metrics.plane_sse``
    accepts, both with one row stride) -> int64 ``[n, Hc, Wc]`` on their device, exact; its sum over the cells is ``plane_sse``'s luma
    entry.  One launch on the current stream; nothing synchronises."""
    import torch

    from . import _lib
    from .frames_out import LAYOUTS, frame_bytes
    from .metrics import _frame_rows
    H, W = int(H), int(W)
    cell = check_cell(cell, "block_sse")
    if fmt.layout == "rgb24":
        raise ValueError("block_sse: rgb24 frames hold no luma plane")
    nbytes = frame_bytes(H, W, fmt)
    a, n, sa = _frame_rows(a_u8, nbytes, fmt, "block_sse")
    b, nb, sb = _frame_rows(b_u8, nbytes, fmt, "block_sse")
    if nb != n or a.device != b.device:
        raise ValueError(f"block_sse: the two buffers must hold the same number of frames on one device (got {n} and {nb})")
    if n > 1 and sa != sb:          # the kernel takes one stride: packed copies
        a, b, sa = a[:, :nbytes].contiguous(), b[:, :nbytes].contiguous(), nbytes
    elif n == 1:
        sa = max(sa, sb)
    Hc, Wc = map_shape(H, W, cell)
    out = torch.empty((n, Hc, Wc), dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().gsvc_frames_block_sse(a.data_ptr(), b.data_ptr(), sa, n, H, W, LAYOUTS[fmt.layout], fmt.depth, cell,
                                                    out.data_ptr(), _lib.current_stream(a.device)), "gsvc_frames_block_sse")
    return out


def weighted_psnr_y(sse_blocks, weights, depth: int, H: int, W: int):
    """``(per frame float64 [n], pooled)``: ``10 log10(peak^2 H W / sum_cells w sse)`` of every frame and
    ``10 log10(peak^2 n H W / sum_frames sum_cells w sse)``, ``peak = 2^depth - 1``, in float64; ``+inf`` where the weighted SSE is 0.
    ``sse_blocks``: int64 ``[n, Hc, Wc]`` (``block_sse``), ``weights``: ``[n, Hc, Wc]`` normalised maps.  With all-ones maps this is
    ``metrics.code_metrics``'s ``psnr_y``.  (H and W are arguments: a map's shape does not tell the size of its partial cells.)"""
    sse, w = _host64(sse_blocks, "weighted_psnr_y"), _host64(weights, "weighted_psnr_y")
    if sse.ndim != 3 or sse.shape != w.shape:
        raise ValueError(f"weighted_psnr_y: sse and weights must be two [n, Hc, Wc] arrays of one shape (got {tuple(sse.shape)} and "
                         f"{tuple(w.shape)})")
    peak2, px = float((1 << int(depth)) - 1) ** 2, float(int(H) * int(W))
    wsse = (w * sse).sum(axis=(1, 2))

    def db(num, den):
        return float("inf") if den <= 0 else 10.0 * float(np.log10(num / den))

    return np.array([db(peak2 * px, v) for v in wsse], dtype=np.float64), db(peak2 * px * sse.shape[0], float(wsse.sum()))
