"""The references of tests/_step_kernel_refs.py pinned on their own, without a GPU: a wrong reference must not be able to bless
a wrong kernel.  ``gen_tail_ref`` against the package's per-render tensor statement of the generation tail and at the three edges
whose convention the kernel has to share (zero quaternion, a Gaussian exactly on a bound, saturated sigmoids); ``adam_ref``
against torch.optim.Adam in float64.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests._step_kernel_refs import EPS32, adam_ref, err, gen_tail_ref, ulp_distance

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def T(a):
    return torch.from_numpy(np.asarray(a))


def test_gen_tail_ref_matches_per_render_statement():
    """float64 gen_tail_ref on the inputs of the tiny model's generation (tests/golden/tiny_model.npz, K = 4) against what
    generate_neural_gaussians computes in fp32 tensor operations: opacity product and mask bit-for-bit (one rounding, and the
    float64 product of two fp32 numbers is exact), sigmoid scaling, normalised rotation and clamped position to 8 eps32 of the
    tensor's scale (at most eight fp32 roundings per output)."""
    from gsvc_amd.arguments import ModelParams
    from gsvc_amd.generate import GenerateMode, _visible_mask, generate_neural_gaussians
    from gsvc_amd.model import GaussianModel
    g = np.load(os.path.join(GOLD, "tiny_model.npz"))
    mp = ModelParams()
    mp.threshold = 0.08
    pc = GaussianModel(mp, feat_dim=8, n_offsets=4, voxel_size=0.001, update_depth=3, update_init_factor=16,
                       update_hierachy_factor=4, use_feat_bank=False, n_features_per_level=2, log2_hashmap_size=9,
                       log2_hashmap_size_2D=11, resolutions_list=(18, 24, 33), resolutions_list_2D=(130, 258), device="cpu")
    sd = {k[4:]: T(g[k]) for k in g.files if k.startswith("sd::")}
    for nm in ("_anchor", "_offset", "_mask", "_anchor_feat", "_scaling", "_rotation", "_opacity"):
        setattr(pc, nm, torch.nn.Parameter(sd[nm].clone(), requires_grad=nm not in ("_rotation", "_opacity")))
    pc.load_state_dict(sd, strict=True)
    pc.update_anchor_bound(float(g["x_lim"]), float(g["y_lim"]), float(g["z_lim"]))
    K = pc.n_offsets
    frame = SimpleNamespace(cam_pos=torch.tensor([0.0, 0.0, float(g["z_cam"])]))
    vis = T(g["visible_mask"])
    with torch.no_grad():
        gss = generate_neural_gaussians(frame, pc, vis, GenerateMode.TRAINING_FULL_PRECISION)
        # the raw opacities (the function returns only their product with the offset mask): same expressions as its own
        idx = vis.nonzero().squeeze(1)
        anchor, feat = pc.get_anchor.index_select(0, idx), pc._anchor_feat.index_select(0, idx)
        ob_view = (anchor - frame.cam_pos)[:, 2:]
        pe = torch.cat([pc.embed_time_fn(torch.zeros_like(ob_view) + frame.cam_pos[-1]), pc.embed_fn(ob_view)], dim=1)
        op_raw = pc.get_opacity_mlp(feat, pe).reshape(-1)
        offset_mask = _visible_mask(pc, idx).reshape(-1)
    ca = gss.concatenated_all          # [grid_scaling 6 | anchor 3 | colour 3 | scale_rot 7 | offsets 3] per Gaussian
    n = ca.shape[0]
    assert n == idx.numel() * K and n > 0 and (offset_mask == 0).any() and (offset_mask != 0).any()
    d = lambda t: t.double()  # noqa: E731
    lo, hi = pc.bound_min_host, pc.bound_max_host
    no, mask, scaling, rot, world, xyz = gen_tail_ref(
        d(op_raw), d(offset_mask), d(ca[:, 19:22]), torch.zeros(n, 3, dtype=torch.float64), d(ca[:, 12:19]), d(ca[::K, 0:6]),
        d(ca[::K, 6:9]), K, lo, hi)
    assert torch.equal(no.float(), gss.neural_opacity) and torch.equal(no, d(gss.neural_opacity))
    assert torch.equal(mask, gss.mask) and mask.any() and not mask.all()
    for nm, ref in (("scaling", scaling), ("rot", rot), ("xyz", xyz)):
        got = getattr(gss, nm)
        e = err(got, ref[mask], float(ref.abs().max()))
        assert got.shape == ref[mask].shape and e <= 8 * EPS32, (nm, e)
    assert torch.equal(xyz, world.clamp(torch.tensor(lo, dtype=torch.float64), torch.tensor(hi, dtype=torch.float64)))


def _edge_inputs(dtype):
    """Two anchors with K = 3.  Gaussian 0: zero quaternion, offsets zero, anchor 0 exactly on the bounds (lo, hi, lo); Gaussian 1:
    scale_rot[:3] = +100; Gaussian 2: -100; anchor 1 is far outside, so Gaussians 3-5 are clamped."""
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    K, lo, hi = 3, (-1.5, -2.0, -0.75), (1.5, 2.0, 0.75)
    op_raw, offset_mask = r(6), torch.tensor([1.0, 0.0, 1.0, 1.0, 0.5, 1.0])
    grid_offsets, neural_offset, scale_rot = 0.1 * r(6, 3), 0.1 * r(6, 3), r(6, 7)
    grid_scaling = torch.rand(2, 6, generator=g) + 0.1
    anchor = torch.tensor([[lo[0], hi[1], lo[2]], [7.0, -7.0, 7.0]])
    grid_offsets[0], neural_offset[0] = 0.0, 0.0
    scale_rot[0, 3:7] = 0.0
    scale_rot[1, 0:3], scale_rot[2, 0:3] = 100.0, -100.0
    ins = [t.to(dtype).requires_grad_(True) for t in (op_raw, offset_mask, grid_offsets, neural_offset, scale_rot, grid_scaling, anchor)]
    return ins, K, lo, hi


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gen_tail_ref_edge_conventions(dtype):
    """What autograd makes of the statement at its edges, in both precisions the GPU tests run it in: rot of a zero quaternion is
    0 and its gradient is g * 1e12 (F.normalize divides by max(|q|, eps)); a Gaussian whose world position is exactly a bound
    receives the gradient of xyz (torch.clamp's mask is inclusive), one outside does not while world's own gradient still
    arrives; sigmoids saturated at +-100 give a finite gradient of (near) zero."""
    ins, K, lo, hi = _edge_inputs(dtype)
    op_raw, offset_mask, grid_offsets, neural_offset, scale_rot, grid_scaling, anchor = ins
    no, mask, scaling, rot, world, xyz = gen_tail_ref(*ins, K, lo, hi)
    assert torch.equal(rot[0], torch.zeros(4, dtype=dtype))
    assert torch.equal(world[0], anchor[0]) and torch.equal(xyz[0], world[0])
    assert torch.equal(mask, torch.tensor([op_raw[0] > 0, False, op_raw[2] > 0, op_raw[3] > 0, op_raw[4] > 0, op_raw[5] > 0]))
    w_rot = torch.tensor([[0.5, -2.0, 3.0, 1.0]], dtype=dtype).expand(6, 4)
    w_xyz = torch.tensor([[2.0, -3.0, 5.0]], dtype=dtype).expand(6, 3)
    w_world = torch.tensor([[0.25, 0.5, -1.0]], dtype=dtype).expand(6, 3)
    (d_sr,) = torch.autograd.grad((rot * w_rot).sum() + scaling.sum(), scale_rot, retain_graph=True)
    assert err(d_sr[0, 3:7], w_rot[0] * 1e12, 1e12) <= 2 * EPS32          # eps = 1e-12 is itself rounded in fp32
    assert torch.isfinite(d_sr).all() and float(d_sr[1:3, 0:3].abs().max()) <= 1e-40
    assert float(d_sr[3:, 0:3].abs().min()) > 1e-3                          # the unsaturated ones do get one
    d_off, d_anchor = torch.autograd.grad((xyz * w_xyz).sum() + (world * w_world).sum(), (grid_offsets, anchor))
    gs = grid_scaling.detach()
    assert torch.equal(d_off[0], (w_xyz[0] + w_world[0]) * gs[0, 0:3])     # on the bound: both arrive
    assert (world[3:] > torch.tensor(hi, dtype=dtype)).logical_or(world[3:] < torch.tensor(lo, dtype=dtype)).all()
    assert torch.equal(d_off[3:], (w_world[3:] * gs[1:2, 0:3]))             # outside: only world's
    assert torch.equal(d_anchor[1], 3 * w_world[0])


def test_adam_ref_matches_torch_adam_float64():
    """adam_ref chained over 5 steps against torch.optim.Adam on float64 parameters.  The two differ only in how the constants
    are rounded (adam_ref takes fp32 betas / eps as the kernel does: relative 3e-8 per constant and step) -> 1e-6 of each tensor's
    scale; a wrong bias correction, a missing square root or eps inside the root are wrong by far more."""
    gen = torch.Generator().manual_seed(11)
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-15
    p0 = torch.randn(301, generator=gen, dtype=torch.float64)
    q = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t in range(1, 6):
        g = torch.randn(301, generator=gen, dtype=torch.float64) * 10.0 ** (t - 3)
        g[::7] = 0.0
        q.grad = g.clone()
        opt.step()
        p, m, v = adam_ref(p, g, m, v, lr, b1, b2, eps, t)
        assert p.dtype == torch.float64
        for got, ref in ((p, q.detach()), (m, opt.state[q]["exp_avg"]), (v, opt.state[q]["exp_avg_sq"])):
            assert err(got, ref, float(ref.abs().max())) <= 1e-6, t
    assert float((p - p0).abs().max()) > 1e-2
    assert torch.isfinite(p).all()


def test_err_and_ulp_distance():
    a = torch.tensor([1.0, -2.0, 0.0, 3.0], dtype=torch.float32)
    b = torch.tensor([1.0, -2.5, 0.0, 3.0], dtype=torch.float32)
    assert err(a, b, 2.0) == 0.25
    assert err(a, b, torch.tensor([1.0, 0.5, 0.0, 1.0])) == 1.0
    assert err(a, b, torch.tensor([1.0, 0.0, 0.0, 1.0])) == float("inf")      # a zero scale demands equality
    assert err(a, a, torch.zeros(4)) == 0.0
    one = torch.tensor([1.0, -1.0, 0.0], dtype=torch.float32)
    nxt = torch.nextafter(one, torch.tensor([2.0, -2.0, 1.0]))
    assert ulp_distance(one, nxt).tolist() == [1, 1, 1]
    assert ulp_distance(torch.tensor([0.0]), torch.tensor([-0.0])).tolist() == [0]
    assert ulp_distance(torch.tensor([-1e-45]), torch.tensor([1e-45])).tolist() == [2]
