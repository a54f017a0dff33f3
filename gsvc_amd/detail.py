"""Content-adaptive initial anchors: where a clip has detail, and points drawn from that.

The reference starts every fit from points drawn uniformly in the cube (frame_cube/utils.py:6-15, init_point_cloud) and leaves it to
densification to move capacity to where the video has structure.  ``new_fit(init="detail")`` replaces that draw (and nothing else:
``GaussianModel.create_from_points`` still merges the points of a voxel and sets every anchor's scale from its 3-NN distance):

  ``luma_detail``     the detail map of a buffer of Y'CbCr frames: per cell of ``cell`` x ``cell`` pixels the sum of the absolute
                      central differences in x and y and twice the absolute difference to the temporal neighbour, in integers on the
                      luma codes (csrc/detail.hip, gsvc_frames_detail).
  ``cube_detail``     that map for every frame of a cube.  A Y'CbCr video file is analysed on its own codes, whatever its residency;
                      every other cube through 16-bit full-range 4:4:4 codes of its float pictures.
  ``sample_points``   ``n`` points from a map: a share ``mix`` uniform over the pixels, the rest in proportion to the cells' detail
                      (csrc/detail.hip, gsvc_detail_sample: a counter-based hash, so the draw is a function of (map, n, mix, seed)).
  ``detail_points``   those points in the cube's world coordinates, as ``create_from_points`` takes them.

``DEFAULT_CELL`` and ``DEFAULT_MIX`` are starting values, not measured ones.
"""
from __future__ import annotations

import numpy as np

from . import _lib

CELLS = (4, 8, 16)
DEFAULT_CELL = 8          # a starting value, not measured
DEFAULT_MIX = 0.25        # the uniform share of the points; a starting value, not measured
INITS = ("uniform", "detail")
CHUNK = 16                # frames per launch of a cube that is analysed in chunks, plus one overlapping frame


def check_cell_mix(cell, mix, what: str = "detail"):
    """``(cell, mix)`` as (int, float) or a ValueError that names the choices."""
    if isinstance(cell, bool) or cell not in CELLS:
        raise ValueError(f"{what}: cell must be one of {', '.join(str(c) for c in CELLS)} (got {cell!r})")
    try:
        m = float(mix)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: mix must be a number in [0, 1] (got {mix!r})") from None
    if not 0.0 <= m <= 1.0:
        raise ValueError(f"{what}: mix must lie in [0, 1] (got {mix!r})")
    return int(cell), m


def map_shape(H: int, W: int, cell: int):
    """``(Hc, Wc)``: the cells of an H x W picture, the last row and column partial where ``cell`` does not divide the side."""
    return -(-int(H) // cell), -(-int(W) // cell)


def luma_detail(frames_u8, H: int, W: int, fmt, cell: int = DEFAULT_CELL, n_out: int | None = None):
    """The detail map of the first ``n_out`` (None: all) frames of a buffer of ``yuv420p`` / ``yuv444p`` frames (what
    ``metrics.picture_hash`` accepts) -> uint32 ``[n_out, Hc, Wc]`` on their device (include/gsvc_hip.h, gsvc_frames_detail).  Frame
    ``n_out - 1`` takes frame ``n_out`` as its temporal neighbour when the buffer has one: a caller that walks a video in chunks
    overlaps them by one frame.  One launch on the current stream; nothing synchronises."""
    import torch

    from .frames_out import LAYOUTS, frame_bytes
    from .metrics import _frame_rows
    H, W = int(H), int(W)
    cell, _ = check_cell_mix(cell, 0.0, "luma_detail")
    if fmt.layout == "rgb24":
        raise ValueError("luma_detail: rgb24 frames hold no luma plane")
    a, n, stride = _frame_rows(frames_u8, frame_bytes(H, W, fmt), fmt, "luma_detail")
    n_out = n if n_out is None else int(n_out)
    if not 1 <= n_out <= n:
        raise ValueError(f"luma_detail: n_out must be 1 .. {n} (got {n_out})")
    Hc, Wc = map_shape(H, W, cell)
    out = torch.empty((n_out, Hc, Wc), dtype=torch.uint32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().gsvc_frames_detail(a.data_ptr(), stride, n, n_out, H, W, LAYOUTS[fmt.layout], fmt.depth, cell, out.data_ptr(),
                                                 _lib.current_stream(a.device)), "gsvc_frames_detail")
    return out


def chunks(T: int):
    """``[(first, n, n_out)]``: windows of up to ``CHUNK + 1`` frames that cover ``T`` frames, each giving the maps of its first
    ``n_out``.  A window that does not reach the end hands its last frame to the next one as that window's first; the window that does
    reach it maps all its frames and always holds two or more (T > 1), so the clip's last frame finds its predecessor."""
    out, s = [], 0
    while True:
        n = min(CHUNK + 1, T - s)
        if s + n >= T:
            out.append((s, n, n))
            return out
        out.append((s, n, CHUNK))
        s += CHUNK


def file_detail(frames, H: int, W: int, fmt, cell: int, device):
    """The map of the frames of an opened video file (host array ``[T, frame_bytes]``), uploaded in the windows of ``chunks`` through
    one pinned staging buffer -> uint32 ``[T, Hc, Wc]`` on ``device``."""
    import torch
    T, nbytes = int(frames.shape[0]), int(frames.shape[1])
    Hc, Wc = map_shape(H, W, cell)
    rows = min(CHUNK + 1, T)
    staging = torch.empty((rows, nbytes), dtype=torch.uint8, pin_memory=True)
    host = staging.numpy()
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        on_dev = torch.empty((rows, nbytes), dtype=torch.uint8, device=device)
        out = torch.empty((T, Hc, Wc), dtype=torch.uint32, device=device)
        for s, n, n_out in chunks(T):
            np.copyto(host[:n], frames[s:s + n])
            on_dev[:n].copy_(staging[:n], non_blocking=True)
            out[s:s + n_out].copy_(luma_detail(on_dev[:n], H, W, fmt, cell, n_out))
            stream.synchronize()          # the staging buffer is free again
    return out


def _float_picture(cube, i: int, device):
    """Frame i of a cube as float32 ``[3, H, W]`` on ``device`` (cubes keep their pictures transposed, ``[3, W, H]``)."""
    from .frame import HostResidentCube
    if isinstance(cube, HostResidentCube):
        img = cube._images[i]          # (its own host copy: fetching through its upload slots would disturb a fit's prefetch)
    else:
        img = cube[i].image
        if hasattr(cube, "ready"):
            cube.ready(i)
    return img.detach().to(device).float().permute(0, 2, 1)


def cube_detail(cube, cell: int = DEFAULT_CELL, device=None):
    """The detail map of every frame of a cube -> uint32 ``[T, Hc, Wc]`` on the cube's device.

    A ``VideoFileCube`` of a Y'CbCr file (also inside an ``EstimatedFlowCube``) analyses the FILE's codes in either residency
    (``VideoFileCube.luma_detail``): the same map, and so the same fit, for both.  A ``frame_range`` cube analyses its own frames only:
    the last frame of a group of pictures looks back, never across the cut.  Every other cube (``SyntheticFrameCube``,
    ``FrameCubeDataset``, ``HostResidentCube``, an ``rgb24`` file) has its float pictures converted to 16-bit full-range BT.709 4:4:4
    codes (``frames_to_u8``) in the windows of ``chunks``."""
    import torch

    from .frames_out import FrameFormat, frames_to_u8
    cell, _ = check_cell_mix(cell, 0.0, "cube_detail")
    fmt = getattr(cube, "fmt", None)
    if fmt is not None and fmt.layout != "rgb24" and hasattr(cube, "luma_detail"):
        return cube.luma_detail(cell)
    dev = torch.device(device if device is not None else getattr(cube, "device", "cuda"))
    if dev.type != "cuda":
        dev = torch.device("cuda", torch.cuda.current_device())
    T, H, W = int(cube.len_z_frames), int(cube.height), int(cube.width)
    codes = FrameFormat("yuv444p", "bt709", "full", depth=16)
    Hc, Wc = map_shape(H, W, cell)
    with torch.cuda.device(dev):
        out = torch.empty((T, Hc, Wc), dtype=torch.uint32, device=dev)
        for s, n, n_out in chunks(T):
            buf = frames_to_u8([_float_picture(cube, s + k, dev) for k in range(n)], codes)
            out[s:s + n_out].copy_(luma_detail(buf, H, W, codes, cell, n_out))
    return out


def mix24_of(mix: float) -> int:
    """The uniform share as the kernel takes it: a point is uniform when 24 bits of its hash are below ``round(mix 2^24)``."""
    return int(round(float(mix) * (1 << 24)))


def sample_points(dmap, H: int, W: int, cell: int = DEFAULT_CELL, n: int = 1, mix: float = DEFAULT_MIX, seed: int = 0):
    """``n`` points from the map ``dmap`` (uint32 ``[T, Hc, Wc]`` on the device) -> ``(points, cell_of, total)``: float32 ``[n, 3]`` =
    (x in pixels, y in pixels, t in frames; pixel k covers [k, k + 1), frame t covers [t - 0.5, t + 0.5)), int32 ``[n]`` = the flat
    cell of each point, and the map's total as a 0-dim int64 tensor (include/gsvc_hip.h, gsvc_detail_sample).  The prefix sum is
    ``torch.cumsum`` in int64; the total is read on the device: nothing synchronises."""
    import torch
    cell, mix = check_cell_mix(cell, mix, "sample_points")
    H, W, n = int(H), int(W), int(n)
    if dmap.dtype != torch.uint32 or dmap.dim() != 3 or not dmap.is_cuda:
        raise ValueError(f"sample_points: the map must be a uint32 CUDA tensor [T, Hc, Wc] (got {dmap.dtype} {tuple(dmap.shape)})")
    if n < 1:
        raise ValueError(f"sample_points: n must be positive (got {n})")
    T = int(dmap.shape[0])
    cdf = torch.cumsum((dmap.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF).reshape(-1), 0)
    points = torch.empty((n, 3), dtype=torch.float32, device=dmap.device)
    cell_of = torch.empty((n,), dtype=torch.int32, device=dmap.device)
    with torch.cuda.device(dmap.device):
        _lib.check(_lib.lib().gsvc_detail_sample(cdf.data_ptr(), int(cdf.shape[0]), T, H, W, cell, n, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                 mix24_of(mix), points.data_ptr(), cell_of.data_ptr(), _lib.current_stream(dmap.device)),
                   "gsvc_detail_sample")
    return points, cell_of, cdf[-1]


def to_world(points, cube) -> np.ndarray:
    """(x px, y px, t frames) -> float64 world coordinates of ``cube``: ``x = x_min + px / scale``, ``y = y_min + py / scale``,
    ``z = (pt - T / 2) / scale``.  The renderer's own ``u = (x - x_min) scale - pix_off`` (csrc/raster_common.h) is the inverse, and
    frame t's camera sits at ``z = (t - T / 2) / scale``."""
    p = np.asarray(points, dtype=np.float64)
    s = float(cube.scale)
    return np.stack([float(cube.x_min) + p[:, 0] / s, float(cube.y_min) + p[:, 1] / s, (p[:, 2] - int(cube.len_z_frames) / 2) / s], axis=1)


def detail_points(cube, n: int, cell: int = DEFAULT_CELL, mix: float = DEFAULT_MIX, seed: int = 0):
    """``n`` initial anchor points of a fit on ``cube`` -> ``(float64 numpy [n, 3] world coordinates, the map's total)``.  All points
    lie inside the pictures and within half a frame of a frame's camera (the uniform draw of the reference bleeds 10 % over every side;
    this one does not).
    Replaces the draw of the reference's init_point_cloud (frame_cube/utils.py:6-15)."""
    dmap = cube_detail(cube, cell)
    points, _, total = sample_points(dmap, int(cube.height), int(cube.width), cell, n, mix, seed)
    return to_world(points.cpu().numpy(), cube), int(total)
