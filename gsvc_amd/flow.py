"""Optical flow from the video itself: a dense estimator on the device (csrc/flow.hip; the algorithm: include/gsvc_hip.h).

The fitting step's flow-guided loss (``loss_utils.calc_optical_loss``) needs one field ``[2, H, W]`` per adjacent frame pair.  The
reference takes these from an external pretrained network; ``estimate_flow`` computes them from the frames: a classical coarse-to-fine
Horn-Schunck with warping, no weights, stencils only, the same bits in every run.  Convention (that of
``SyntheticFrameCube.get_optical_flow`` and of the loss): ``flow[0]`` = x displacement, ``flow[1]`` = y displacement in pixels at the
pixel of frame t, ``I_t(x, y) ~ I_{t+1}(x + flow[0], y + flow[1])``; float32 ``[2, H, W]``.

``EstimatedFlowCube`` wraps any frame cube and answers ``get_optical_flow`` from the cube's own pictures.  The kernels need the built
library and a GPU (no CPU fallback); importing this module does not.
"""
from __future__ import annotations

import dataclasses
import os
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

CHUNK = 16                  # pairs per call: bounds the workspace (about 47 bytes per pixel and pair), as the frame stages' chunks do
LUMA_WEIGHTS = (0.2126, 0.7152, 0.0722)


@dataclass(frozen=True)
class FlowParams:
    alpha: float = 0.02      # weight of the smoothness term (pictures in [0, 1])
    warps: int = 5           # warps per pyramid level
    iters: int = 30          # Jacobi sweeps per warp
    min_side: int = 8        # no pyramid level has a shorter side
    max_levels: int = 6
    max_step: float = 1.0    # a warp moves a pixel's flow by at most this much per component (pixels of the level)


def luma(x: torch.Tensor) -> torch.Tensor:
    """``[..., 3, H, W]`` RGB in [0, 1] -> ``[..., H, W]``: 0.2126 R + 0.7152 G + 0.0722 B."""
    r, g, b = LUMA_WEIGHTS
    return r * x[..., 0, :, :] + g * x[..., 1, :, :] + b * x[..., 2, :, :]


def _planes(x, what: str):
    """``[H, W]`` luma, ``[3, H, W]`` picture, ``[n, 1, H, W]`` lumas or ``[n, 3, H, W]`` pictures -> (float32 ``[n, H, W]``, batched?)."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"estimate_flow: {what} must be a tensor (got {type(x).__name__})")
    if not x.is_cuda:
        raise _lib.GsvcError("estimate_flow runs on the HIP kernels of csrc/flow.hip; CPU tensors are not supported")
    x = x.float()
    if x.dim() == 2:
        return x.unsqueeze(0), False
    if x.dim() == 3 and x.shape[0] == 3:
        return luma(x).unsqueeze(0), False
    if x.dim() == 4 and x.shape[1] == 1:
        return x[:, 0], True
    if x.dim() == 4 and x.shape[1] == 3:
        return luma(x), True
    raise ValueError(f"estimate_flow: {what} must be [H, W], [3, H, W], [n, 1, H, W] or [n, 3, H, W] (got {tuple(x.shape)})")


def _run(l0: torch.Tensor, l1: torch.Tensor, pitch: int, n: int, H: int, W: int, p: FlowParams, out: torch.Tensor):
    """gsvc_flow_estimate on n pairs starting at the first elements of l0 and l1, ``pitch`` floats apart, into ``out`` [n, 2, H, W]."""
    L = _lib.lib()
    need = int(L.gsvc_flow_workspace_bytes(n, H, W, p.max_levels, p.min_side))
    if need < 0:
        raise ValueError(f"estimate_flow: {H} x {W} with min_side {p.min_side}, max_levels {p.max_levels}: sides must be 2 .. 32768 and at "
                         f"least min_side (>= 2)")
    ws = torch.empty(need, dtype=torch.uint8, device=out.device)
    with torch.cuda.device(out.device):
        _lib.check(L.gsvc_flow_estimate(l0.data_ptr(), l1.data_ptr(), pitch, n, H, W, float(p.alpha), int(p.warps), int(p.iters),
                                        int(p.min_side), int(p.max_levels), float(p.max_step), out.data_ptr(), ws.data_ptr(),
                                        _lib.current_stream(out.device)), "gsvc_flow_estimate")


def _params(params) -> FlowParams:
    p = params.pop("params", None)
    if p is not None and params:
        raise ValueError("estimate_flow: give either params=FlowParams(...) or its fields as keywords")
    return p if p is not None else FlowParams(**params)


def estimate_flow(a: torch.Tensor, b: torch.Tensor, **params) -> torch.Tensor:
    """The flow from ``a`` to ``b``: float32 ``[2, H, W]``, or ``[n, 2, H, W]`` for batches.  ``a`` and ``b``: CUDA ``[H, W]`` luma in [0, 1],
    ``[3, H, W]`` RGB pictures, or batches ``[n, 1, H, W]`` / ``[n, 3, H, W]``.  Keywords: the fields of ``FlowParams`` (or ``params=``).
    Long batches run ``CHUNK`` pairs at a time; a pair's result does not depend on the batch.  Nothing synchronises."""
    p = _params(dict(params))
    la, batched = _planes(a, "a")
    lb, batched_b = _planes(b, "b")
    if la.shape != lb.shape or batched != batched_b or la.device != lb.device:
        raise ValueError(f"estimate_flow: a and b must have the same shape on one device (got {tuple(a.shape)} and {tuple(b.shape)})")
    la, lb = la.contiguous(), lb.contiguous()
    n, H, W = (int(v) for v in la.shape)
    out = torch.empty((n, 2, H, W), dtype=torch.float32, device=la.device)
    for i in range(0, n, CHUNK):
        m = min(CHUNK, n - i)
        _run(la[i:], lb[i:], H * W, m, H, W, p, out[i:])
    return out if batched else out[0]


def sequence_flow(lumas: torch.Tensor, **params) -> torch.Tensor:
    """CUDA float32 contiguous ``[T, H, W]`` lumas of T frames -> ``[T - 1, 2, H, W]``: pair k = frames k, k + 1, read where they lie."""
    p = _params(dict(params))
    if not lumas.is_cuda:
        raise _lib.GsvcError("sequence_flow runs on the HIP kernels of csrc/flow.hip; CPU tensors are not supported")
    if lumas.dim() != 3 or lumas.dtype != torch.float32 or not lumas.is_contiguous() or lumas.shape[0] < 2:
        raise ValueError(f"sequence_flow: lumas must be contiguous float32 [T >= 2, H, W] (got {lumas.dtype} {tuple(lumas.shape)})")
    T, H, W = (int(v) for v in lumas.shape)
    out = torch.empty((T - 1, 2, H, W), dtype=torch.float32, device=lumas.device)
    for i in range(0, T - 1, CHUNK):
        m = min(CHUNK, T - 1 - i)
        _run(lumas[i:], lumas[i + 1:], H * W, m, H, W, p, out[i:])
    return out


def save_flows(flows, directory) -> list:
    """One ``flow_%05d.npy`` per field under ``directory`` (created), float32 ``[2, H, W]``: ``io.load_flow`` reads each back bit for bit,
    and the directory serves as ``optical_flow_dir`` of ``VideoFileCube`` / ``io.FrameCubeDataset`` (sorted by name = by pair).  Returns
    the paths."""
    os.makedirs(directory, exist_ok=True)
    paths = []
    for k, f in enumerate(flows):
        path = os.path.join(str(directory), f"flow_{k:05d}.npy")
        np.save(path, f.detach().to("cpu", torch.float32).contiguous().numpy(), allow_pickle=False)
        paths.append(path)
    return paths


class EstimatedFlowCube:
    """A frame cube (``VideoFileCube``, ``io.FrameCubeDataset``, ``SyntheticFrameCube``, ...) whose optical flow is estimated from its
    own pictures: the T - 1 fields are computed once, here, and stay on the device as float32 (8 bytes per pixel and pair: 16.6 MB per
    1080p pair, 1 GB for 64 frames).  ``get_optical_flow(i)`` hands out field i; everything else (``cube[i]``, ``get_z_frame``,
    ``get_dummy_frame``, ``ready``, ``luma_detail``, ``fmt``, ``scale``, ``x_min``, ...) is the wrapped cube's.  The cube's pictures are ``[3, W, H]`` (transposed,
    as the reference keeps them); the estimator is given ``[H, W]``.  ``Trainer``, ``HostResidentCube`` and ``report.evaluate`` take it
    as they take the cube."""

    def __init__(self, cube, device=None, **params):
        self.cube = cube
        self.flow_params = _params(dict(params))
        T = int(cube.len_z_frames)
        if T < 2:
            raise ValueError("EstimatedFlowCube: a cube of fewer than two frames has no frame pair")
        first = cube[0].image
        dev = torch.device(device) if device is not None else (first.device if first.is_cuda else torch.device("cuda", torch.cuda.current_device()))
        H, W = int(cube.height), int(cube.width)
        lumas = torch.empty((T, H, W), dtype=torch.float32, device=dev)
        for i in range(T):
            img = cube[i].image
            if hasattr(cube, "ready"):
                cube.ready(i)          # (a cube that uploads ahead: the picture has landed before it is read)
            img = img.to(dev)
            if tuple(img.shape) != (3, W, H):
                raise ValueError(f"EstimatedFlowCube: frame {i} is {tuple(img.shape)}, not the transposed [3, {W}, {H}]")
            lumas[i].copy_(luma(img.float()).permute(1, 0))
        self.flows = sequence_flow(lumas, params=self.flow_params)

    def __getattr__(self, name):          # (only what this object does not have itself)
        if name == "cube":
            raise AttributeError(name)
        return getattr(self.cube, name)

    def __len__(self):
        return len(self.cube)

    def __getitem__(self, idx):
        return self.cube[idx]

    def get_optical_flow(self, idx):
        return self.flows[idx]

    def save_flows(self, directory) -> list:
        return save_flows(self.flows, directory)

    def describe(self) -> dict:
        """What a log should say about where the flow came from."""
        return {"source": "estimated", "params": dataclasses.asdict(self.flow_params), "pairs": int(self.flows.shape[0])}
