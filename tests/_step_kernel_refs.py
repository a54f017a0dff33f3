"""Plain tensor statements of the training step's elementwise kernels, written from the kernels' header comments
(csrc/generate.hip, csrc/adam.hip).  Called with float64 tensors they are the references of tests/test_gen_tail_gpu.py and
tests/test_film_adam_gpu.py; called with float32 tensors they are "the fp32 tensor statement" those tests calibrate against.
tests/test_step_kernel_refs_cpu.py pins them without a GPU.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = float(np.finfo(np.float32).eps)       # 2^-23
PRINT = bool(os.environ.get("GSVC_PRINT_ERRORS"))


def gen_tail_expanded(op_raw, offset_mask, grid_offsets, neural_offset, scale_rot, gs_rep, anchor_rep, lo, hi):
    """The five formulas per Gaussian, with the anchor row's grid_scaling [n, 6] / anchor [n, 3] already repeated per Gaussian
    (as leaves, their gradients are the K terms of the row sums that d_grid_scaling / d_anchor add up)."""
    n = scale_rot.shape[0]
    dt, dev = scale_rot.dtype, scale_rot.device
    neural_opacity = op_raw.reshape(n, 1) * offset_mask.reshape(n, 1)
    mask = (neural_opacity > 0).view(-1)
    scaling = gs_rep[:, 3:6] * torch.sigmoid(scale_rot[:, 0:3])
    rot = F.normalize(scale_rot[:, 3:7], dim=1, eps=1e-12)
    world = anchor_rep + (grid_offsets.reshape(n, 3) + neural_offset.reshape(n, 3)) * gs_rep[:, 0:3]
    xyz = torch.clamp(world, torch.as_tensor(lo, dtype=dt, device=dev), torch.as_tensor(hi, dtype=dt, device=dev))
    return neural_opacity, mask, scaling, rot, world, xyz


def gen_tail_ref(op_raw, offset_mask, grid_offsets, neural_offset, scale_rot, grid_scaling, anchor, K, lo, hi):
    """(neural_opacity [n, 1], mask [n], scaling [n, 3], rot [n, 4], world [n, 3], xyz [n, 3]) for n = rows * K Gaussians, in the
    dtype of the inputs, differentiable."""
    return gen_tail_expanded(op_raw, offset_mask, grid_offsets, neural_offset, scale_rot,
                             grid_scaling.repeat_interleave(K, dim=0), anchor.repeat_interleave(K, dim=0), lo, hi)


def adam_ref(p, g, m, v, lr, b1, b2, eps, t):
    """One Adam update in float64, returns (p, m, v).  b1, b2, eps are rounded to fp32 first and 1 - beta is rounded to fp32 from
    double, as csrc/adam.hip states:
        m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    The bias corrections are those of the host side (double, from the unrounded betas, then fp32)."""
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    bc1, bc2 = f32(1.0 - b1 ** t), f32(1.0 - b2 ** t)
    omb1, omb2 = f32(1.0 - b1), f32(1.0 - b2)
    b1, b2, eps, lr = f32(b1), f32(b2), f32(eps), f32(lr)
    p, g, m, v = (x.double() for x in (p, g, m, v))
    m = b1 * m + omb1 * g
    v = b2 * v + omb2 * g * g
    p = p - (lr / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + eps))
    return p, m, v


def err_each(got, ref, scale):
    """|got - ref| / scale per element in float64; ``scale``: a positive number or a tensor broadcastable against ``ref`` (zero
    entries of a tensor scale require an exact match there: 0 / 0 counts as 0, x / 0 as inf)."""
    d = (got.double() - ref.double()).abs()
    if not torch.is_tensor(scale):
        assert scale > 0, scale
        return d / scale
    scale = scale.double().expand_as(d)
    return torch.where(scale > 0, d / scale.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))


def err(got, ref, scale):
    """max |got - ref| / scale (see err_each), 0 for empty tensors."""
    q = err_each(got, ref, scale)
    return float(q.max()) if q.numel() else 0.0


def ulp_distance(a, b):
    """Distance of two finite float32 tensors in units in the last place (int64), through the ordered-integer view of IEEE floats."""
    def key(x):
        i = x.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(b)).abs()
