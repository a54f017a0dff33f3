"""GPU parity of the hash-grid and entropy-rate HIP kernels (through the C-ABI) against the oracles and the
golden vectors captured from the reference's Python.  Tolerances: grid forward/dy_dx 1e-6 abs on O(1) values
(fp32, FMA contraction differs from the oracle), table gradients 1e-5 relative (float atomics reorder sums),
rate bits 2e-3 (fp32 erf cancellation, same size as the reference-vs-float64 gap) and gradients 2e-3 relative.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False)


def C(a, dtype=None):
    t = torch.tensor(np.asarray(a), device="cuda")
    return t.to(dtype) if dtype is not None else t


def _levels(D, res, log2):
    from gsvc_amd.encodings import level_offsets
    return np.array(level_offsets(res, D, log2), dtype=np.int32), np.array(res, dtype=np.int32)


@pytest.mark.parametrize("D,Cf,res,log2,N", [(3, 8, (18, 24, 33, 44, 59, 80), 13, 5000), (2, 8, (130, 258, 514), 15, 4097),
                                              (3, 2, (6, 9, 14), 9, 333), (2, 4, (10, 18), 8, 64), (1, 1, (16, 64), 5, 100),
                                              (3, 16, (18, 40), 11, 257), (2, 32, (20,), 7, 65),
                                              # tables too large for 16 LDS slices: the global-atomic fallback of k_grid_bwd_lds
                                              (3, 2, (64, 128, 256), 19, 20000), (2, 1, (1026, 2050), 21, 5000),
                                              # the production tables of cfg_20240919.yaml in full (reference
                                              # scene/gaussian_model.py:280-281, arguments/__init__.py:68-70): 12 3-D levels up to
                                              # resolution 514 with 2^13 rows, 4 2-D levels up to 1026 with 2^15 rows, 8 features
                                              (3, 8, (18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514), 13, 30000),
                                              (2, 8, (130, 258, 514, 1026), 15, 30000)])
def test_grid_kernels_match_oracle(oracle_lib, D, Cf, res, log2, N):
    from gsvc_amd import gridencoder_backend as be
    rng = np.random.default_rng(D * 100 + Cf)
    off, rs = _levels(D, res, log2)
    L = len(res)
    emb = np.sign(rng.standard_normal((off[-1], Cf))).astype(np.float32)
    emb[emb == 0] = 1
    x = rng.uniform(0, 1, (N, D)).astype(np.float32)
    x[0] = 0.0
    x[1] = 1.0
    x[2, 0] = -0.1
    x[3, -1] = 1.0001
    x[4] = 0.5
    ref_out, ref_dy = oracle_lib.grid_forward(x, emb, off, rs, calc_dy_dx=True)
    out = torch.empty(L, N, Cf, device="cuda")
    dy = torch.empty(N, L * D * Cf, device="cuda")
    be.grid_encode_forward(C(x), C(emb), C(off), C(rs), out, N, D, Cf, L, 0, 128, 0, dy, None, None)
    assert np.abs(out.cpu().numpy() - ref_out).max() < 1e-6
    assert np.abs(dy.cpu().numpy() - ref_dy).max() < 1e-4 * max(res)   # dy_dx scales with the resolution
    assert np.all(out.cpu().numpy()[:, 2] == 0) and np.all(out.cpu().numpy()[:, 3] == 0)
    # no dy_dx requested
    out2 = torch.empty(L, N, Cf, device="cuda")
    be.grid_encode_forward(C(x), C(emb), C(off), C(rs), out2, N, D, Cf, L, 0, 128, 0, None, None, None)
    assert torch.equal(out, out2)
    # backward
    g = rng.standard_normal((L, N, Cf)).astype(np.float32)
    ref_ge, ref_gi = oracle_lib.grid_backward(g, x, emb, off, rs, ref_dy)
    ge = torch.zeros(off[-1], Cf, device="cuda")
    gi = torch.zeros(N, D, device="cuda")
    be.grid_encode_backward(C(g), C(x), C(emb), C(off), C(rs), ge, N, D, Cf, L, 0, 128, C(ref_dy), gi, None, None)
    assert np.abs(ge.cpu().numpy() - ref_ge).max() < 1e-5 * max(1.0, np.abs(ref_ge).max())
    assert np.abs(gi.cpu().numpy() - ref_gi).max() < 1e-5 * max(1.0, np.abs(ref_gi).max())
    # accumulate semantics: a second call adds on top (reference encodings.py:574 zero-fills per call)
    be.grid_encode_backward(C(g), C(x), C(emb), C(off), C(rs), ge, N, D, Cf, L, 0, 128, None, None, None, None)
    assert np.abs(ge.cpu().numpy() - 2 * ref_ge).max() < 2e-5 * max(1.0, np.abs(ref_ge).max())


def test_grid_table_backward_fixed_point_range_determinism_and_nonfinite(oracle_lib):
    """k_grid_bwd_lds sums a table slice in 64-bit fixed point scaled by the level's largest |grad| (csrc/grid.hip): a
    contribution is resolved to 2^-47 of that or better, so entries six orders of magnitude below the level's largest
    gradient still carry float accuracy; levels are scaled apart; two launches give the same bits (one chunk of points: the
    slice sums do not depend on the order of the adds); a non-finite gradient propagates the way the float path did."""
    from gsvc_amd import gridencoder_backend as be
    D, Cf, res, log2, N = 3, 8, (18, 24, 33, 44), 13, 2000
    rng = np.random.default_rng(11)
    off, rs = _levels(D, res, log2)
    L = len(res)
    emb = np.ones((off[-1], Cf), dtype=np.float32)
    x = rng.uniform(0.05, 0.95, (N, D)).astype(np.float32)
    g = rng.standard_normal((L, N, Cf)).astype(np.float32)
    g[..., 0] *= 1e3                 # channel 0 carries each level's largest gradients
    g[..., 1] *= 1e-3                # channel 1 is six orders of magnitude below them
    g[..., 2] = 0.0
    g[3] *= 1e-12                    # a level whose gradients are all tiny keeps its own scale
    g[2] *= 1e-25                    # ... and one below 2^-60 takes the float path
    ref_ge, _ = oracle_lib.grid_backward(g, x, emb, off, rs, None)
    outs = []
    for _ in range(2):
        ge = torch.zeros(off[-1], Cf, device="cuda")
        be.grid_encode_backward(C(g), C(x), C(emb), C(off), C(rs), ge, N, D, Cf, L, 0, 128, None, None, None, None)
        outs.append(ge)
    fixed = np.r_[0:off[2], off[3]:off[4]]                                   # rows of the levels summed in fixed point
    assert torch.equal(outs[0][fixed], outs[1][fixed])
    got = outs[0].cpu().numpy()
    for lvl in range(L):
        for ch in range(Cf):         # per level and channel, relative to that block's own scale
            a, b = got[off[lvl]:off[lvl + 1], ch], ref_ge[off[lvl]:off[lvl + 1], ch]
            assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max() + 0.0, (lvl, ch)
    assert np.all(got[:, 2] == 0)
    # every gradient zero: nothing is added
    ge = torch.zeros(off[-1], Cf, device="cuda")
    be.grid_encode_backward(torch.zeros(L, N, Cf, device="cuda"), C(x), C(emb), C(off), C(rs), ge, N, D, Cf, L, 0, 128, None, None, None, None)
    assert not ge.any()
    # one NaN / inf in the incoming gradient reaches the rows that point touches (its level takes the float path)
    for bad in (np.nan, np.inf):
        g2 = g.copy()
        g2[1, 7, 3] = bad
        ge = torch.zeros(off[-1], Cf, device="cuda")
        be.grid_encode_backward(C(g2), C(x), C(emb), C(off), C(rs), ge, N, D, Cf, L, 0, 128, None, None, None, None)
        got = ge.cpu().numpy()
        assert (~np.isfinite(got[off[1]:off[2], 3])).sum() >= 1 and np.isfinite(np.delete(got, 3, axis=1)).all()
        fin = np.isfinite(got[:, 3])
        assert np.abs(got[fin, 3] - ref_ge[fin, 3]).max() <= 1e-5 * np.abs(ref_ge[:, 3]).max()


def test_param_means_match_torch():
    """csrc/rate.hip k_param_means against the three torch reductions it replaces (x_mean of the rate's clamp bounds)."""
    from types import SimpleNamespace
    from gsvc_amd.generate import _param_means
    torch.manual_seed(2)
    A = 100_003
    pc = SimpleNamespace(_anchor_feat=torch.randn(A, 50, device="cuda") + 0.3, _scaling=torch.randn(A, 6, device="cuda") * 0.5 - 3.0,
                         _offset=torch.randn(A, 10, 3, device="cuda") * 0.1, decoded_version=False)
    pc.get_scaling = torch.exp(pc._scaling)
    got = _param_means(pc).double().cpu()
    want = torch.stack([pc._anchor_feat.double().mean(), pc.get_scaling.double().mean(), pc._offset.double().mean()]).cpu()
    assert ((got - want).abs() <= 2e-6 * want.abs() + 1e-7).all(), (got, want)
    assert torch.equal(_param_means(pc), _param_means(pc))            # fixed order
    pc.decoded_version = True
    assert abs(float(_param_means(pc)[1]) - float(pc._scaling.double().mean())) <= 2e-6 * abs(float(pc._scaling.double().mean()))


def test_grid_backend_error_behaviour():
    from gsvc_amd import _lib
    from gsvc_amd import gridencoder_backend as be
    off, rs = _levels(3, (6, 9), 9)
    x = torch.rand(10, 3, device="cuda")
    emb = torch.ones(int(off[-1]), 3, device="cuda")       # 3 features: unsupported
    out = torch.empty(2, 10, 3, device="cuda")
    with pytest.raises(RuntimeError, match="n_fearures must be 1, 2, 4, 8, 16 or 32"):
        be.grid_encode_forward(x, emb, C(off), C(rs), out, 10, 3, 3, 2, 0, 128, 0, None, None, None)
    with pytest.raises(RuntimeError, match="num_dim must be 1, 2, 3"):
        be.grid_encode_forward(torch.rand(10, 4, device="cuda"), torch.ones(int(off[-1]), 2, device="cuda"), C(off), C(rs),
                               torch.empty(2, 10, 2, device="cuda"), 10, 4, 2, 2, 0, 128, 0, None, None, None)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        be.grid_encode_forward(x.cpu(), emb, C(off), C(rs), out, 10, 3, 3, 2, 0, 128, 0, None, None, None)
    with pytest.raises(RuntimeError, match="must be a contiguous tensor"):
        be.grid_encode_forward(torch.rand(3, 10, device="cuda").t(), emb, C(off), C(rs), out, 10, 3, 3, 2, 0, 128, 0, None, None, None)
    with pytest.raises(RuntimeError, match="must be an int tensor"):
        be.grid_encode_forward(x, emb, C(off).long(), C(rs), out, 10, 3, 3, 2, 0, 128, 0, None, None, None)
    assert issubclass(_lib.GsvcError, RuntimeError)
    # empty batch is a no-op
    be.grid_encode_forward(torch.empty(0, 3, device="cuda"), torch.ones(int(off[-1]), 2, device="cuda"), C(off), C(rs),
                           torch.empty(2, 0, 2, device="cuda"), 0, 3, 2, 2, 0, 128, 0, None, None, None)


@pytest.mark.parametrize("tag,D,res,log2,Cf", [("3d", 3, (6, 9, 14, 20), 9, 4), ("2d", 2, (10, 18, 34), 8, 8)])
def test_grid_encoder_module_matches_reference_fixture(tag, D, res, log2, Cf):
    """Our GridEncoder (STE_binary + autograd wrapper + HIP kernels) against the reference's GridEncoder driving
    the oracle backend."""
    from gsvc_amd.encodings import GridEncoder
    g = load("grid_encoder_" + tag)
    enc = GridEncoder(num_dim=D, n_features=Cf, resolutions_list=res, log2_hashmap_size=log2).cuda()
    assert enc.offsets_list.tolist() == g["offsets"].tolist()
    enc.params.data.copy_(C(g["params"]))
    x = C(g["x"]).requires_grad_(True)
    out = enc(x)
    assert np.abs(out.detach().cpu().numpy() - g["out"]).max() < 1e-6
    (out * C(g["gout"])).sum().backward()
    assert np.abs(enc.params.grad.cpu().numpy() - g["dparams"]).max() < 1e-5 * max(1.0, np.abs(g["dparams"]).max())
    assert np.abs(x.grad.cpu().numpy() - g["dx"]).max() < 1e-4 * max(1.0, np.abs(g["dx"]).max())


def test_rate_kernels_match_reference_and_oracle():
    from gsvc_amd.entropy_models import EntropyGaussian
    from oracle import rate_oracle as ro
    g = load("rate_entropy_gaussian")
    x, mean, scale, Q = (C(g[k]).requires_grad_(True) for k in ("x", "mean", "scale", "Q"))
    eg = EntropyGaussian(Q=1)
    bits = eg(x, mean, scale, Q, C(g["x_mean"]))
    b = bits.detach().cpu().numpy()
    assert np.array_equal(b == 16.0, g["bits"] == 16.0)
    if os.environ.get("GSVC_PRINT_ERRORS"):
        print(f"RATE_ERR bits {np.abs(b - g['bits']).max():.3e} of {np.abs(g['bits']).max():.3e}")
    assert np.abs(b - g["bits"]).max() < 2e-4            # measured 6e-5 (of 16 bits: the fp32 erfc difference near the 2^-16 floor)
    (bits * C(g["gout"])).sum().backward()
    for t, nm in ((x, "dx"), (mean, "dmean"), (scale, "dscale"), (Q, "dQ")):
        ref = g[nm]
        if os.environ.get("GSVC_PRINT_ERRORS"):
            print(f"RATE_ERR {nm} {np.abs(t.grad.cpu().numpy() - ref).max() / np.abs(ref).max():.3e}")
        assert np.abs(t.grad.cpu().numpy() - ref).max() < 1e-4 * np.abs(ref).max(), nm          # measured 9e-6
    assert np.all(mean.grad.cpu().numpy()[g["bits"] == 16.0] == 0)   # Low_bound net rule
    assert x.grad[2, 0].item() == 0                                       # clamped x gets no gradient
    # scalar Q, x_mean taken from x
    bs = eg(C(g["x"]), C(g["mean"]), C(g["scale"]), 0.2, None).cpu().numpy()
    ok = g["bits_scalar_q"] < 15.9
    assert np.abs(bs - g["bits_scalar_q"])[ok].max() < 2e-3
    # random larger shape against the float64 oracle, 3-D input with broadcast Q
    rng = np.random.default_rng(5)
    n, c = 3000, 50
    xr = rng.standard_normal((n, c)).astype(np.float32) * 2
    mr = rng.standard_normal((n, c)).astype(np.float32)
    sr = (rng.uniform(0.05, 2, (n, c))).astype(np.float32)
    qr = rng.uniform(0.05, 1.0, (n, 1)).astype(np.float32)
    ref_bits, _, _, _ = ro.entropy_gaussian_bits(xr, mr, sr, qr, float(xr.mean()))
    ours = eg(C(xr), C(mr), C(sr), C(qr), None).cpu().numpy()
    # vs the float64 oracle: fp32 erf differences are amplified where the likelihood is tiny (the reference's
    # own fp32 chain has the same gap); vs the same chain in plain fp32 PyTorch on the GPU: tight
    assert np.abs(ours - ref_bits).max() < 5e-2 and np.median(np.abs(ours - ref_bits)) < 1e-5
    m1 = torch.distributions.normal.Normal(C(mr), C(sr))
    xc = torch.clamp(C(xr), min=float(xr.mean() - 15000 * qr.mean()), max=float(xr.mean() + 15000 * qr.mean()))
    lik = torch.clamp(m1.cdf(xc + 0.5 * C(qr)) - m1.cdf(xc - 0.5 * C(qr)), min=2 ** -16)
    torch_bits = (-torch.log2(lik)).cpu().numpy()
    assert np.abs(ours - torch_bits).max() < 2e-3
    # empty selection (a 5 % sample can be empty) returns an empty tensor
    e = eg(torch.empty(0, 6, device="cuda"), torch.empty(0, 6, device="cuda"), torch.empty(0, 6, device="cuda"),
           torch.empty(0, 1, device="cuda"), torch.tensor(0.0, device="cuda"))
    assert e.shape == (0, 6)
    with pytest.raises(RuntimeError):
        eg(torch.zeros(2, 2), torch.zeros(2, 2), torch.ones(2, 2), 1.0)   # CPU tensors: no fallback


class Replay:
    """Replays the reference run's random tensors (recorded by make_golden.py) on the GPU."""

    def __init__(self, tape):
        self.tape = list(tape)
        self._rand_like, self._uniform = torch.rand_like, torch.Tensor.uniform_

    def __enter__(self):
        tape = self.tape

        def rand_like(x, *a, **k):
            return torch.tensor(tape.pop(0), device=x.device).view_as(x)

        def uniform_(t, *a, **k):
            return t.copy_(torch.tensor(tape.pop(0), device=t.device).view_as(t))

        torch.rand_like, torch.Tensor.uniform_ = rand_like, uniform_
        return self

    def __exit__(self, *exc):
        torch.rand_like, torch.Tensor.uniform_ = self._rand_like, self._uniform


@pytest.fixture(scope="module")
def tiny_gpu():
    from gsvc_amd.arguments import ModelParams
    from gsvc_amd.model import GaussianModel
    g = load("tiny_model")
    mp = ModelParams()
    mp.threshold = 0.08
    pc = GaussianModel(mp, feat_dim=8, n_offsets=4, voxel_size=0.001, update_depth=3, update_init_factor=16,
                       update_hierachy_factor=4, use_feat_bank=False, n_features_per_level=2, log2_hashmap_size=9,
                       log2_hashmap_size_2D=11, resolutions_list=(18, 24, 33), resolutions_list_2D=(130, 258), device="cuda")
    sd = {k[4:]: C(g[k]) for k in g.files if k.startswith("sd::")}
    for nm in ("_anchor", "_offset", "_mask", "_anchor_feat", "_scaling", "_rotation", "_opacity"):
        setattr(pc, nm, torch.nn.Parameter(sd[nm].clone(), requires_grad=nm not in ("_rotation", "_opacity")))
    pc.load_state_dict(sd, strict=True)
    pc.update_anchor_bound(float(g["x_lim"]), float(g["y_lim"]), float(g["z_lim"]))
    return pc, g


def test_entropy_context_matches_reference(tiny_gpu):
    pc, g = tiny_gpu
    vis = C(g["visible_mask"])
    anchor = pc.get_anchor[vis]
    assert np.abs(pc.calc_interp_feat(anchor).detach().cpu().numpy() - g["interp_feat"]).max() < 1e-6
    ec = pc.calc_entropy_context(anchor)
    for nm in ("mean_feat", "scale_feat", "mean_scaling", "scale_scaling", "mean_offsets", "scale_offsets",
               "Q_feat_adj", "Q_scaling_adj", "Q_offsets_adj"):
        ref = g["ec::" + nm]
        assert np.abs(getattr(ec, nm).detach().cpu().numpy() - ref).max() < 2e-5 * max(1.0, np.abs(ref).max()), nm


@pytest.mark.parametrize("mode_value", [0, 1, 2, 3])
def test_generate_all_modes_on_gpu(tiny_gpu, mode_value):
    from gsvc_amd.generate import GenerateMode, generate_neural_gaussians
    pc, g = tiny_gpu
    pre = f"gen{mode_value}::"
    frame = SimpleNamespace(cam_pos=torch.tensor([0.0, 0.0, float(g["z_cam"])]))
    tape = [g[pre + f"rand{i}"] for i in range(int(g[pre + "n_rand"]))]
    with Replay(tape) as rp:
        gss = generate_neural_gaussians(frame, pc, C(g["visible_mask"]), GenerateMode(mode_value))
        assert len(rp.tape) == 0   # same number and order of random draws as the reference
    assert np.array_equal(gss.mask.cpu().numpy(), g[pre + "mask"])
    for nm in ("xyz", "color", "opacity", "scaling", "rot", "neural_opacity"):
        ref = g[pre + nm]
        assert np.abs(getattr(gss, nm).detach().cpu().numpy() - ref).max() < 3e-5 * max(1.0, np.abs(ref).max()), nm
    if mode_value >= 2:
        for nm in ("bit_per_param", "bit_per_feat_param", "bit_per_scaling_param", "bit_per_offsets_param"):
            ref = float(g[pre + nm])
            assert abs(float(getattr(gss, nm)) - ref) < 2e-4 * max(1.0, abs(ref)), nm
        # the rate is differentiable down to the hash tables and the entropy nets
        if mode_value == 2:
            pc.zero_grad()
            gss.bit_per_param.backward()
            assert pc.encoding_xyz.encoding_xyz.params.grad.abs().sum() > 0
            assert pc.mlp_feature_enet.dist_net[0].weight.grad.abs().sum() > 0
            assert pc._anchor_feat.grad.abs().sum() > 0
    else:
        assert gss.bit_per_param is None


def test_render_end_to_end_matches_oracle_raster(tiny_gpu, oracle_lib):
    """render() = prefilter -> generate -> rasterize; the image equals the oracle rasterizer fed with the
    generated Gaussians, the visible mask equals the oracle's visible_filter, gradients reach the anchors."""
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.generate import GenerateMode
    from gsvc_amd.ortho_gaussian_renderer import prefilter_voxel, render
    pc, g = tiny_gpu
    cube = SyntheticFrameCube(54, 96, 60)
    frame = cube.get_dummy_frame(33)
    pipe = SimpleNamespace(debug=False, compute_cov3D_python=False)
    bg = torch.tensor([0.0, 0.0, 0.0])
    pc.zero_grad()
    res = render(frame, pc, pipe, bg, retain_grad=True, mode=GenerateMode.TRAINING_FULL_PRECISION)
    st = oracle_lib.make_settings(54, 96, frame.x_min, frame.y_min, frame.scale, pc.model_config.threshold,
                                  frame.view_matrix.permute(1, 0).contiguous().numpy())
    anchors = pc.get_anchor.detach().cpu().numpy()
    radii, _, _ = oracle_lib.raster_preprocess(st, anchors, pc.get_scaling[:, :3].detach().cpu().numpy(),
                                               pc.get_rotation.detach().cpu().numpy())
    assert np.array_equal(res.visible_mask.cpu().numpy(), radii > 0)
    assert torch.equal(prefilter_voxel(frame, pc, pipe, bg), res.visible_mask)
    gs = res.generated_gaussians
    ref = oracle_lib.raster_forward(st, gs.xyz.detach().cpu().numpy(), gs.color.detach().cpu().numpy(),
                                    gs.opacity.detach().cpu().numpy(), gs.scaling.detach().cpu().numpy(),
                                    gs.rot.detach().cpu().numpy())
    assert res.num_rendered == ref.num_rendered and int(res.active_gaussains) == int((ref.radii > 0).sum())
    ok = ref.borderline == 0
    assert np.abs(res.rendered_image.detach().cpu().numpy() - ref.image)[:, ok].max() < 1e-4
    res.rendered_image.sum().backward()
    assert res.viewspace_points.grad is not None and res.viewspace_points.grad.abs().sum() > 0
    assert pc._anchor_feat.grad.abs().sum() > 0 and pc._offset.grad.abs().sum() > 0 and pc._scaling.grad.abs().sum() > 0


def test_compat_install_provides_the_native_module_names():
    import importlib
    import sys
    from gsvc_amd import compat
    compat.install(renderer=True)
    be = importlib.import_module("_gridencoder")
    assert hasattr(be, "grid_encode_forward") and hasattr(be, "grid_encode_backward")
    ras = importlib.import_module("diff_gaussian_rasterization.cuda_ortho_gaussian_rasterizer")
    assert hasattr(ras, "GaussianRasterizationSettings") and hasattr(ras, "GaussianRasterizer")
    ogr = importlib.import_module("ortho_gaussian_renderer")
    for nm in ("render", "prefilter_voxel", "generate_neural_gaussians", "GenerateMode", "GeneratedGaussians", "RatePack",
               "calc_sampled_rate"):
        assert hasattr(ogr, nm)
    assert hasattr(importlib.import_module("gaussian_renderer"), "render")
    for k in ("_gridencoder", "diff_gaussian_rasterization", "diff_gaussian_rasterization.cuda_ortho_gaussian_rasterizer",
              "ortho_gaussian_renderer", "gaussian_renderer"):
        sys.modules.pop(k, None)


@pytest.mark.parametrize("H,W", [(48, 64), (37, 53), (16, 16), (5, 7)])
def test_fused_ssim_l1_matches_torch_and_reference(H, W):
    """csrc/ssim.hip vs the plain PyTorch fp32 statement of the same op (five 11x11 depthwise convs) and, at
    48x64, vs the reference's own numbers (tests/golden/image_losses.npz).  fp32: 2e-6 on the means, 1e-5
    relative on the gradient."""
    import torch.nn.functional as F
    from gsvc_amd import loss_utils as LU
    if (H, W) == (48, 64):
        g = load("image_losses")
        a, b = C(g["img1"]), C(g["img2"])
    else:
        gen = torch.Generator().manual_seed(H * 100 + W)
        a = torch.rand(3, H, W, generator=gen).cuda()
        b = (a + 0.2 * torch.randn(3, H, W, generator=gen).cuda()).clamp(0, 1)
    a.requires_grad_(True)
    s, l = LU.ssim_l1(a, b)
    (0.2 * (1 - s) + 0.8 * l).backward()
    ga = a.grad.clone()
    # plain torch reference on the GPU
    a2 = a.detach().clone().requires_grad_(True)
    w1 = LU._window_1d(11, 1.5).cuda()
    w2 = (w1[:, None] @ w1[None, :]).expand(3, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t.unsqueeze(0), w2, padding=5, groups=3)[0]  # noqa: E731
    mu1, mu2 = conv(a2), conv(b)
    s1, s2, s12 = conv(a2 * a2) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a2 * b) - mu1 * mu2
    smap = ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    s_ref, l_ref = smap.mean(), (a2 - b).abs().mean()
    (0.2 * (1 - s_ref) + 0.8 * l_ref).backward()
    assert abs(float(s) - float(s_ref)) < 2e-6 and abs(float(l) - float(l_ref)) < 1e-7
    assert (ga - a2.grad).abs().max() < 1e-5 * a2.grad.abs().max() + 1e-9
    if (H, W) == (48, 64):
        assert abs(float(s) - float(g["ssim"])) < 2e-6 and abs(float(l) - float(g["l1"])) < 1e-7
        assert abs(float(LU.ssim_func(a.detach(), b)) - float(g["ssim"])) < 2e-6
        per = LU.ssim_func(a.detach().unsqueeze(0), b.unsqueeze(0), size_average=False)
        assert np.abs(per.cpu().numpy() - g["ssim_per"]).max() < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(48, 64), (70, 100)])
def test_ssim_l1_pair_equals_the_averaged_frame(H, W):
    """ssim_l1 with ``img_b`` forms the two-view frame (f + flip_W(b)) / 2 inside the kernels: same losses, same frame and the same gradients
    for both views as averaging first and calling it without."""
    from gsvc_amd import loss_utils as LU
    gen = torch.Generator().manual_seed(H + W)
    f = torch.rand(3, H, W, generator=gen).cuda().requires_grad_(True)
    b = torch.rand(3, H, W, generator=gen).cuda().requires_grad_(True)
    gt = torch.rand(3, H, W, generator=gen).cuda()
    s, l, avg = LU.ssim_l1(f, gt, img_b=b)
    (0.2 * (1 - s) + 0.8 * l).backward()
    got = (f.grad.clone(), b.grad.clone())
    f.grad = b.grad = None
    img = (f + torch.flip(b, dims=(-1,))) / 2
    s2, l2 = LU.ssim_l1(img, gt)
    (0.2 * (1 - s2) + 0.8 * l2).backward()
    assert torch.equal(avg, img.detach()) and not avg.requires_grad
    assert float(s) == float(s2) and float(l) == float(l2)
    assert torch.allclose(got[0], f.grad, rtol=1e-6, atol=1e-12) and torch.allclose(got[1], b.grad, rtol=1e-6, atol=1e-12)


@pytest.mark.gpu
def test_counted_ste_binary_and_table_bits():
    """STE_binary_counted = STE_binary + the number of +1 entries; the hash-bit term computed from those counts equals the
    reference-style expression on the concatenated tables (value and gradient)."""
    from gsvc_amd.encodings import STE_binary, STE_binary_counted
    from gsvc_amd.train import _TableBits, get_binary_vxl_size_device
    torch.manual_seed(2)
    ps = [(torch.randn(n, 8, device="cuda") * 0.7).requires_grad_(True) for n in (1000, 777, 3001)]
    with torch.no_grad():
        ps[0][:5] = 0.0                      # zeros binarise to +1
    outs = [STE_binary_counted.apply(p) for p in ps]
    for p, (y, c) in zip(ps, outs):
        assert torch.equal(y, STE_binary.apply(p.detach())) and float(c) == float((p.detach() >= 0).sum())
    bits = _TableBits.apply(torch.cat([c for _, c in outs]), *[y for y, _ in outs])
    bits.backward()
    got = [p.grad.clone() for p in ps]
    for p in ps:
        p.grad = None
    ref = get_binary_vxl_size_device((torch.cat([STE_binary.apply(p) for p in ps], 0) + 1) / 2)
    ref.backward()
    assert abs(float(bits) - float(ref)) <= 1e-6 * float(ref)
    for a, p in zip(got, ps):
        # (autograd differentiates through p = n1 / n as well: terms that cancel analytically leave ~1e-6 of float32 noise)
        assert (a - p.grad).abs().max().item() <= 1e-5 * p.grad.abs().max().item() + 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("R,rows,empty", [(4, 5000, None), (2, 700, None), (4, 900, 2), (1, 300, None)])
def test_rate_normalise_matches_tensor_expression(R, rows, empty):
    """k_rate_normalise (keep rates from the offset masks, sample sizes from the sorted row list, per-group and overall bits
    per parameter, their sum) = the tensor expression of reference guassian.py:110-132 per render, values and gradient; a render
    without sampled rows gives the same NaN / inf as the expression."""
    from gsvc_amd.generate import _RateNorm
    torch.manual_seed(R * 1000 + rows)
    K, dev = 10, "cuda"
    cuts = sorted(torch.randint(1, rows, (R - 1,)).tolist())
    bounds = [0] + cuts + [rows]
    om = (torch.rand(rows, K, 1, device=dev) < 0.12).float()
    pick = torch.rand(rows, device=dev) < 0.07
    if empty is not None:
        pick[bounds[empty]:bounds[empty + 1]] = False
    sel = pick.nonzero().squeeze(1)
    S = (torch.rand(R, 3, device=dev) * 1e4).requires_grad_(True)
    dims = (50.0, 6.0, 30.0)
    out, total = _RateNorm.apply(S, om, sel, bounds, dims, K)
    w = torch.randn(R, 4, device=dev)
    ok = torch.ones(R, dtype=torch.bool, device=dev)
    if empty is not None:
        ok[empty] = False
    ((out * w)[ok].sum() + (0.0 if empty is not None else 0.5 * total)).backward()
    got = S.grad.clone()
    S.grad = None
    live = om.sum(dim=1)[:, 0] > 0
    bt = torch.tensor(bounds, device=dev)
    cnt = (bt[1:] - bt[:-1]).float()
    kr = torch.stack([live[bounds[r]:bounds[r + 1]].sum() for r in range(R)]).float() / cnt.clamp_min(1)
    edges = torch.searchsorted(sel, bt)
    N = (edges[1:] - edges[:-1]).float().unsqueeze(1) * torch.tensor(dims, device=dev)
    per = S / N * kr.unsqueeze(1)
    tot = S.sum(dim=1) / N.sum(dim=1) * kr
    ref = torch.cat([tot.unsqueeze(1), per], dim=1)
    ((ref * w)[ok].sum() + (0.0 if empty is not None else 0.5 * tot.sum())).backward()
    assert torch.allclose(out[ok], ref[ok], rtol=1e-6, atol=0)
    if empty is None:
        assert abs(float(total) - float(tot.sum())) <= 1e-6 * float(tot.sum())
    else:
        assert not torch.isfinite(out[empty]).any() or float(S[empty].abs().sum()) == 0
    assert torch.allclose(got[ok], S.grad[ok], rtol=1e-5, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("R,A", [(4, 5000), (2, 333), (6, 1200)])
def test_film_row_maps_match_tensor_expression(R, A):
    """gsvc_film_row_maps = the index arithmetic it replaces (gsvc_amd.generate._film_rows): FiLM row of every chain row and,
    per (frame, distinct anchor), the chain rows of the two opposite views (-1 where a view does not see the anchor)."""
    import ctypes as C
    from gsvc_amd import _lib
    torch.manual_seed(R * A)
    dev = "cuda"
    M = torch.rand(R, A, device=dev) < 0.3
    M[1] = M[0] ^ (torch.rand(A, device=dev) < 0.05)        # opposite views see almost the same anchors
    present = M.any(dim=0)
    distinct = present.nonzero().squeeze(1)
    D = int(distinct.shape[0])
    pos = torch.cumsum(present, 0) - 1
    c = torch.cumsum(M.view(-1), 0)
    vis_list = [M[r].nonzero().squeeze(1) for r in range(R)]
    vis = torch.cat(vis_list)
    bounds = [0]
    for v in vis_list:
        bounds.append(bounds[-1] + int(v.shape[0]))
    rows, F = bounds[-1], R // 2
    maps = torch.full((rows + 2 * F * D,), -7, dtype=torch.int32, device=dev)
    row_of, src_a, src_b = maps[:rows], maps[rows:rows + F * D], maps[rows + F * D:]
    _lib.check(_lib.lib().gsvc_film_row_maps(_lib.ptr(vis), (C.c_int64 * (R + 1))(*bounds), R, _lib.ptr(pos), D, A, _lib.ptr(M), _lib.ptr(c),
                                             _lib.ptr(distinct), _lib.ptr(row_of), C.c_void_p(src_a.data_ptr()), C.c_void_p(src_b.data_ptr()),
                                             _lib.current_stream(torch.device(dev))), "gsvc_film_row_maps")
    seg_id = torch.repeat_interleave(torch.arange(R, device=dev), torch.tensor([b - a for a, b in zip(bounds[:-1], bounds[1:])], device=dev))
    ref_row = (pos[vis] + (seg_id // 2) * D).int()
    base = (torch.arange(R, device=dev) * A).view(R, 1) + distinct.view(1, D)
    ref = torch.where(M.view(-1)[base.view(-1)], c[base.view(-1)] - 1, torch.full((), -1, device=dev, dtype=c.dtype)).view(F, 2, D).int()
    assert torch.equal(row_of, ref_row)
    assert torch.equal(src_a.view(F, D), ref[:, 0]) and torch.equal(src_b.view(F, D), ref[:, 1])
    # every chain row is the source of exactly one FiLM row entry
    both = torch.cat([src_a, src_b])
    assert torch.equal(both[both >= 0].sort().values, torch.arange(rows, device=dev, dtype=torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("R,A,sample", [(4, 50007, True), (1, 4096, True), (3, 4097, False), (5, 13, True), (2, 8192, True), (4, 244860, True)])
def test_plan_scans_match_cumsum_and_nonzero(R, A, sample):
    """gsvc_plan_scans (three launches) = cumsum / nonzero of the flattened view masks, of the union mask and of the rate sample:
    chunk boundaries inside views, views that are not multiples of the 16-byte loads, empty and full masks."""
    import ctypes as C
    from gsvc_amd import _lib
    torch.manual_seed(R * A)
    dev = "cuda"
    M = torch.rand(R, A, device=dev) < 0.35
    if R >= 3:
        M[1] = False
        M[2] = True
    present = M.any(dim=0)
    chosen = (M & (torch.rand(R, A, device=dev) < 0.2)) if sample else None
    L = _lib.lib()
    big = torch.full((3 * R * A + 2 * A + R + 2,), -5, dtype=torch.int64, device=dev)
    c, flat, sel = big[:R * A], big[R * A:2 * R * A], big[2 * R * A:3 * R * A]
    pos, distinct, counts = big[3 * R * A:3 * R * A + A], big[3 * R * A + A:3 * R * A + 2 * A], big[3 * R * A + 2 * A:]
    scratch = torch.empty(int(L.gsvc_plan_scans_scratch_bytes(R, A)), dtype=torch.uint8, device=dev)
    v = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(L.gsvc_plan_scans(_lib.ptr(M), _lib.ptr(chosen), _lib.ptr(present), R, A, _lib.ptr(scratch), v(c), v(flat), v(sel) if sample else None,
                                 v(pos), v(distinct), v(counts), _lib.current_stream(torch.device(dev))), "gsvc_plan_scans")
    ref_c = torch.cumsum(M.view(-1), 0)
    assert torch.equal(c, ref_c)
    assert torch.equal(pos, torch.cumsum(present, 0) - 1)
    n = counts.tolist()
    ends = ref_c[A - 1::A].tolist()
    assert n[:R] == ends and n[R] == (int(chosen.sum()) if sample else 0) and n[R + 1] == int(present.sum())
    nz = M.view(-1).nonzero().squeeze(1)
    assert torch.equal(flat[:ends[-1]], nz % A)
    assert torch.equal(distinct[:n[R + 1]], present.nonzero().squeeze(1))
    if sample:
        assert torch.equal(sel[:n[R]], ref_c[chosen.view(-1).nonzero().squeeze(1)] - 1)


@pytest.mark.gpu
def test_q_rows_match_gather_and_product():
    """_QRows = base step x adjustment gathered by context row, for the three groups; gradient = scatter-add onto the distinct rows;
    without a row map the rows are the context rows."""
    from gsvc_amd.generate import _QRows
    torch.manual_seed(3)
    D, rows, dev = 700, 2500, "cuda"
    for with_map in (True, False):
        adj = [(torch.rand(D, 1, device=dev) + 0.5).requires_grad_(True) for _ in range(3)]
        ctx_row = torch.randint(0, D, (rows,), device=dev) if with_map else None
        n = rows if with_map else D
        ws = [torch.randn(n, 1, device=dev) for _ in range(3)]
        qs = (1, 0.001, 0.2)
        out = _QRows.apply(*adj, ctx_row, *qs)
        sum((o * w).sum() for o, w in list(zip(out, ws))[:2]).backward()          # the third output: no gradient
        got = [a.grad for a in adj]
        assert got[2] is None or float(got[2].abs().max()) == 0.0
        ref_adj = [a.detach().clone().requires_grad_(True) for a in adj]
        ref = [q * (a if ctx_row is None else a.index_select(0, ctx_row)) for q, a in zip(qs, ref_adj)]
        sum((o * w).sum() for o, w in list(zip(ref, ws))[:2]).backward()
        for o, r in zip(out, ref):
            assert o.shape == r.shape and torch.equal(o, r)
        for g, a in list(zip(got, ref_adj))[:2]:
            assert torch.allclose(g, a.grad, rtol=1e-5, atol=1e-7)


@pytest.mark.gpu
def test_training_statis_kernel_matches_index_adds():
    """gsvc_training_statis = clamp + sums + gradient norms + four index_adds (reference scene/gaussian_model.py:1281-1314 through
    the nested masks), anchors repeated over the rows as the four views of a step repeat them."""
    import ctypes as C
    from gsvc_amd import _lib
    torch.manual_seed(11)
    A, K, rows, dev = 3000, 10, 7001, "cuda"
    vis = torch.randint(0, A, (rows,), device=dev)
    op = torch.randn(rows * K, 1, device=dev)
    seen = torch.rand(rows * K, device=dev) < 0.4
    g = torch.randn(rows * K, 3, device=dev)
    accs = [torch.rand(A, 1, device=dev), torch.full((A, 1), 3.0, device=dev), torch.rand(A * K, 1, device=dev), torch.zeros(A * K, 1, device=dev)]
    ref = [a.double() for a in accs]
    o = op.double().view(-1).clamp_min(0).view(-1, K)
    ref[0].index_add_(0, vis, o.sum(dim=1, keepdim=True))
    ref[1].index_add_(0, vis, torch.ones(rows, 1, device=dev, dtype=torch.float64))
    w = seen.double().view(-1, K)
    ref[2].view(A, K).index_add_(0, vis, torch.norm(g[:, :2].double(), dim=-1).view(-1, K) * w)
    ref[3].view(A, K).index_add_(0, vis, w)
    _lib.check(_lib.lib().gsvc_training_statis(_lib.ptr(vis), _lib.ptr(op), _lib.ptr(seen), _lib.ptr(g), 3, rows, K,
                                               *[_lib.ptr(a) for a in accs], _lib.current_stream(torch.device(dev))), "gsvc_training_statis")
    for a, r in zip(accs, ref):
        assert torch.allclose(a.double(), r, rtol=2e-6, atol=1e-6)
    assert torch.equal(accs[3], ref[3].float()) and torch.equal(accs[1], ref[1].float())      # counts: exact


@pytest.mark.gpu
def test_tables_binarised_in_one_launch_with_count_bits():
    """STE_binary_tables (all tables in one launch, differentiable counts) + CountBits = the per-table STE_binary and the
    reference-style bit expression on the concatenated tables; the tables also feed another consumer (as the grid lookups do),
    one of them none (gradient through its count only), and sizes straddle the 4096-entry blocks."""
    from gsvc_amd.encodings import STE_binary, STE_binary_tables, CountBits
    from gsvc_amd.train import get_binary_vxl_size_device
    torch.manual_seed(5)
    ps = [(torch.randn(n, 8, device="cuda") * 0.9).requires_grad_(True) for n in (1000, 512, 3001, 1)]
    with torch.no_grad():
        ps[1][:3] = 0.0
    ws = [torch.randn_like(p) for p in ps]

    def loss(embs, bits):
        return 1e-3 * bits + sum((e * w).sum() for e, w in list(zip(embs, ws))[:3])     # the last table: count only

    *ys, counts = STE_binary_tables.apply(*ps)
    for p, y, c in zip(ps, ys, counts):
        assert torch.equal(y, STE_binary.apply(p.detach())) and float(c) == float((p.detach() >= 0).sum())
    bits = CountBits.apply(counts, sum(p.numel() for p in ps))
    loss(ys, bits).backward()
    got = [p.grad.clone() for p in ps]
    for p in ps:
        p.grad = None
    es = [STE_binary.apply(p) for p in ps]
    ref = get_binary_vxl_size_device((torch.cat(es, 0) + 1) / 2)
    loss(es, ref).backward()
    assert abs(float(bits) - float(ref)) <= 1e-6 * float(ref)
    for a, p in zip(got, ps):
        assert (a - p.grad).abs().max().item() <= 1e-5 * p.grad.abs().max().item() + 1e-9
    # no bit term at all: the plain straight-through gradient
    for p in ps:
        p.grad = None
    *ys, _ = STE_binary_tables.apply(*ps)
    sum((e * w).sum() for e, w in zip(ys, ws)).backward()
    for p, w in zip(ps, ws):
        assert torch.equal(p.grad, w * (p.detach().abs() <= 1))


@pytest.mark.parametrize("M,K,N", [(5000, 50, 100), (4097, 116, 100), (8192, 192, 150), (4096, 100, 10), (6000, 66, 66),
                                    (4500, 50, 1), (4096, 8, 16), (70000, 100, 70), (4103, 51, 37), (9001, 192, 192),
                                    (5000, 3, 100), (4099, 150, 192), (4111, 177, 33), (300000, 100, 100),
                                    # weight-gradient blocks of 1, 2 and 3 column tiles, rows aligned to 4 bytes only
                                    (4100, 17, 23), (4101, 81, 49), (4097, 33, 129), (4098, 130, 82)])
def test_mfma_linear_matches_torch(M, K, N):
    """csrc/linear.hip (fp32 MFMA, tall-skinny) vs torch.nn.functional.linear in fp32 on the same GPU: fp32
    products and accumulation on both sides, only the summation order differs -> 1e-5 relative to the row scale.
    This goes through the modules (4096 rows and more); the kernels themselves, from one row on, per element against float64 and
    bit for bit on integer inputs, are checked in tests/test_linear_kernels_gpu.py."""
    import torch.nn.functional as F
    from gsvc_amd.model import Linear
    gen = torch.Generator().manual_seed(M + K + N)
    lin = Linear(K, N).cuda()
    x = torch.randn(M, K, generator=gen).cuda().requires_grad_(True)
    y = lin(x)
    ref = F.linear(x, lin.weight, lin.bias)
    scale = ref.abs().max().item()
    assert (y - ref).abs().max().item() < 1e-5 * max(1.0, scale) * (K ** 0.5)
    g = torch.randn(M, N, generator=gen).cuda()
    (y * g).sum().backward()
    gx, gw, gb = x.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone()
    x.grad = None
    lin.zero_grad()
    (F.linear(x, lin.weight, lin.bias) * g).sum().backward()
    assert torch.allclose(gx, x.grad, rtol=1e-4, atol=1e-5)
    assert torch.allclose(gw, lin.weight.grad, rtol=1e-3, atol=1e-3 * lin.weight.grad.abs().max().item())
    assert torch.allclose(gb, lin.bias.grad, rtol=1e-3, atol=1e-3 * lin.bias.grad.abs().max().item())
    # small batches and CPU tensors keep the library path
    assert torch.equal(lin(x[:10]), F.linear(x[:10], lin.weight, lin.bias))
    # Linear -> ReLU fused into the store, and its backward
    x.grad = None
    lin.zero_grad()
    yr = lin.forward_relu(x)
    assert torch.equal(yr, torch.relu(y.detach()))
    (yr * g).sum().backward()
    gx2, gw2 = x.grad.clone(), lin.weight.grad.clone()
    x.grad = None
    lin.zero_grad()
    # a pre-activation within rounding of 0 may land on either side of the ReLU in the two summation orders, so
    # the reference applies the mask of the fused output
    gm = g * (yr.detach() > 0)
    (F.linear(x, lin.weight, lin.bias) * gm).sum().backward()
    assert torch.allclose(gx2, x.grad, rtol=1e-4, atol=1e-5)
    assert torch.allclose(gw2, lin.weight.grad, rtol=1e-3, atol=1e-3 * lin.weight.grad.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", [(1, "cube"), (3, "cube"), (4, "cube"), (5000, "cube"), (5000, "flat"), (5000, "clustered"),
                                     (20000, "slab")])
def test_knn3_mean_dist2_matches_brute_force(n, shape):
    """csrc/knn.hip (stands in for simple_knn.distCUDA2): exact 3-NN mean squared distance."""
    import numpy as np
    from gsvc_amd.model import mean_3nn_dist2
    rng = np.random.default_rng(n)
    if shape == "cube":
        p = rng.uniform(-1, 1, (n, 3))
    elif shape == "flat":
        p = np.concatenate([rng.uniform(-1, 1, (n, 2)), np.zeros((n, 1))], 1)          # zero extent along z
    elif shape == "clustered":
        p = np.concatenate([rng.normal(0, 0.01, (n // 2, 3)), rng.uniform(-1, 1, (n - n // 2, 3))])   # very uneven cells
    else:
        p = rng.uniform([-1.0, -0.5625, -0.03], [1.0, 0.5625, 0.03], (n, 3))           # GSVC's thin z-slab of anchors
    p32 = p.astype(np.float32)
    got = mean_3nn_dist2(torch.from_numpy(p32).cuda()).cpu().numpy()
    ref = np.empty(n, np.float64)
    P = p32.astype(np.float64)
    for s in range(0, n, 2048):
        d = ((P[s:s + 2048, None, :] - P[None, :, :]) ** 2).sum(-1)
        d[np.arange(d.shape[0]), np.arange(s, s + d.shape[0])] = np.inf
        k = min(3, n - 1)
        ref[s:s + 2048] = np.sort(d, 1)[:, :k].mean(1) if k > 0 else 0.0
    assert np.allclose(got, ref, rtol=2e-5, atol=1e-12), np.abs(got - ref).max()


@pytest.mark.gpu
def test_fused_sampled_rate_matches_the_tensor_path(monkeypatch):
    """k_rate_sample (gathers + per-render clamp bounds + offset mask + per-render sums in one launch, dense-gradient scatter in
    backward) against the same quantities computed with index_select / _GaussianBits / index_add: the four rates of every render
    and the gradient of every input."""
    from gsvc_amd.generate import _Segments, _rate_many
    from gsvc_amd.model import EntropyContext
    dev = torch.device("cuda")
    torch.manual_seed(7)
    K, F = 10, 50
    counts = [3000, 2500, 0, 3100]
    M, D = sum(counts), 4000
    seg = _Segments(counts, dev)
    pc = SimpleNamespace(n_offsets=K, _anchor_feat=torch.randn(9000, F, device=dev), get_scaling=torch.rand(9000, 6, device=dev) * 0.01,
                         _offset=torch.randn(9000, K, 3, device=dev) * 0.1)

    def leaf(*shape, scale=1.0, shift=0.0):
        return (torch.randn(*shape, device=dev) * scale + shift).requires_grad_(True)

    def make():
        torch.manual_seed(11)
        t = dict(feat=leaf(M, F, scale=2.0), gs=leaf(M, 6, scale=0.004, shift=0.01), go=leaf(M, K, 3, scale=0.3),
                 om=(torch.rand(M, K, 1, device=dev) > 0.3).float().requires_grad_(True),
                 qf=(torch.rand(M, 1, device=dev) * 0.5 + 0.75).requires_grad_(True),
                 qs=(torch.rand(M, 1, device=dev) * 0.001 + 0.0005).requires_grad_(True),
                 qo=(torch.rand(M, 1, device=dev) * 0.1 + 0.15).requires_grad_(True),
                 mf=leaf(D, F), sf=(torch.rand(D, F, device=dev) + 0.5).requires_grad_(True), ms=leaf(D, 6, scale=0.004, shift=0.01),
                 ss=(torch.rand(D, 6, device=dev) * 0.004 + 0.001).requires_grad_(True), mo=leaf(D, 3 * K, scale=0.3),
                 so=(torch.rand(D, 3 * K, device=dev) * 0.3 + 0.05).requires_grad_(True))
        return t

    ec_row = torch.randint(0, D, (M,), device=dev)
    live = torch.ones(M, dtype=torch.bool, device=dev)
    sel = ((torch.rand(M, device=dev) < 0.08) & live).nonzero().squeeze(1)
    w = torch.randn(len(counts), 4, device=dev)

    def run(fused):
        if fused:
            monkeypatch.delenv("GSVC_NO_FUSED_RATE", raising=False)
        else:
            monkeypatch.setenv("GSVC_NO_FUSED_RATE", "1")
        t = make()
        ec = EntropyContext(t["mf"], t["sf"], t["ms"], t["ss"], t["mo"], t["so"], None, None, None)
        packs = _rate_many(pc, seg, t["feat"], t["gs"], t["go"], t["om"], t["qf"], t["qs"], t["qo"], ec, ec_row=ec_row, sel=sel)
        vals = torch.stack([torch.stack([p.bit_per_param, p.bit_per_feat_param, p.bit_per_scaling_param, p.bit_per_offsets_param])
                            for p in packs])
        live_r = torch.tensor([c > 0 for c in counts], device=dev)
        (vals[live_r] * w[live_r]).sum().backward()
        return vals.detach(), {k: v.grad for k, v in t.items()}

    v0, g0 = run(False)
    v1, g1 = run(True)
    ok = torch.isfinite(v0)
    assert torch.equal(ok, torch.isfinite(v1))
    assert torch.allclose(v1[ok], v0[ok], rtol=2e-5, atol=1e-6)
    for k in g0:
        assert (g0[k] is None) == (g1[k] is None), k
        if g0[k] is not None:
            scale = g0[k].abs().max().item()
            assert (g1[k] - g0[k]).abs().max().item() <= 2e-4 * scale + 1e-12, (k, scale)


@pytest.mark.gpu
def test_mix_encoding_strided_layout_equals_the_module_path(monkeypatch):
    """Mix3d2dEncoding through gsvc_grid_*_ex (every grid reads its columns of x and writes / reads its column block of the
    [N, 192] matrix) against the per-grid modules + slices + permutes + cat: same features, same table gradients."""
    from gsvc_amd.model import Mix3d2dEncoding
    torch.manual_seed(4)
    enc = Mix3d2dEncoding(n_features=8, resolutions_list=(18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514), log2_hashmap_size=13,
                          resolutions_list_2D=(130, 258, 514, 1026), log2_hashmap_size_2D=15, ste_binary=True, ste_multistep=False,
                          add_noise=False, Q=1).cuda()
    with torch.no_grad():
        for p in enc.parameters():
            p.copy_(torch.randn_like(p))
    N = 20011
    x = torch.rand(N, 3, device="cuda")
    x[0] = 0.0
    x[1] = 1.0
    x[2, 1] = -0.2                                   # outside the cube: zero features, no gradient
    w = torch.randn(N, enc.output_dim, device="cuda")
    from gsvc_amd import _lib
    res = []
    # the four grids in one launch each way (gsvc_grid_*_many) | one launch per grid (gsvc_grid_*_ex) | the per-grid modules
    for form in ("many", "per_grid", "modules"):
        monkeypatch.delenv("GSVC_NO_FUSED_GRID", raising=False)
        monkeypatch.delenv("GSVC_NO_GRID_MANY", raising=False)
        if form == "per_grid":
            monkeypatch.setenv("GSVC_NO_GRID_MANY", "1")
        elif form == "modules":
            monkeypatch.setenv("GSVC_NO_FUSED_GRID", "1")
        enc.zero_grad()
        _lib.profile_enable(True)
        try:
            y = enc(x)
            assert ("MixGridEncode" in type(y.grad_fn).__name__) == (form != "modules")
            (y * w).sum().backward()
            prof = _lib.profile_collect()
        finally:
            _lib.profile_enable(False)
        launches = {k: v[0] for k, v in prof.items() if k.startswith("k_grid")}
        assert launches == ({"k_grid_fwd_many": 1, "k_grid_bwd_many": 1} if form == "many" else {"k_grid_fwd": 4, "k_grid_bwd": 4}), launches
        res.append((y.detach().clone(), [p.grad.clone() for p in enc.parameters()]))
    assert res[0][0].shape == (N, 192) and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][0], res[2][0])
    for other in (res[1][1], res[2][1]):
        for a, b in zip(res[0][1], other):
            assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item() + 1e-9        # float atomics reorder the sums


@pytest.mark.gpu
def test_bit_packed_tables_give_the_float_tables_lookup(monkeypatch):
    """Inference through bit-packed tables (one byte per row of 8 features: gsvc_pack_sign_bits + gsvc_grid_forward_packed) is
    the lookup in the binarised float tables bit for bit: every level of the 3-D and the 2-D grids, points on the cube's faces
    and outside it, zeros in the tables (binarise to +1)."""
    from gsvc_amd.model import Mix3d2dEncoding
    torch.manual_seed(9)
    enc = Mix3d2dEncoding(n_features=8, resolutions_list=(18, 24, 33, 44, 59, 80, 108, 148, 201, 275, 376, 514), log2_hashmap_size=13,
                          resolutions_list_2D=(130, 258, 514, 1026), log2_hashmap_size_2D=15, ste_binary=True, ste_multistep=False,
                          add_noise=False, Q=1).cuda()
    with torch.no_grad():
        for p in enc.parameters():
            p.copy_(torch.randn_like(p))
            p[::7] = 0.0
    N = 30001
    x = torch.rand(N, 3, device="cuda")
    x[0] = 0.0
    x[1] = 1.0
    x[2, 2] = 1.3
    with torch.no_grad():
        packed = enc(x)
        monkeypatch.setenv("GSVC_NO_PACKED_GRID", "1")
        plain = enc(x)
    assert packed.shape == (N, 192) and torch.equal(packed, plain)
    # z outside the cube: the 3-D grid (first 96 columns) and the xz / yz grids give zeros, the xy grid does not
    assert float(packed[2, :96].abs().sum()) == 0.0 and float(packed[2, 96:128].abs().sum()) > 0 and float(packed[2, 128:].abs().sum()) == 0.0
    monkeypatch.delenv("GSVC_NO_PACKED_GRID")
    y = enc(x)                                      # with autograd the float tables are used (their gradient is needed)
    assert "MixGridEncode" in type(y.grad_fn).__name__ and torch.equal(y.detach(), packed)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,per_row_q", [((20000, 50), True), ((20000, 6), True), ((12000, 10, 3), True), ((9000, 50), False)])
def test_fused_ste_quantiser_equals_the_tensor_expression(monkeypatch, shape, per_row_q):
    """gsvc_ste_quant_forward (STE_multistep over the rows of the step's renders: per-render mean step, truncated bounds, clamp, round)
    against the tensor expression it replaces (gsvc_amd/generate.py _seg_ste; reference utils/encodings.py:395-420): bit for bit, with
    rows beyond the 15 000-step bound in the data (the clamp is active) and both forms of the step (per row / one number)."""
    import gsvc_amd.generate as G
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(shape, device="cuda", generator=g) * 3.0
    rows = shape[0]
    Q = (torch.rand(rows, device="cuda", generator=g) * 0.5 + 1e-3).view([rows] + [1] * (len(shape) - 1)) if per_row_q else 0.2
    x[5] = 3.0e4          # far beyond mean / mean(Q) + 15000 steps for small steps
    x[7] = -3.0e4
    x_mean = x.mean()
    seg = G._Segments([rows // 4, rows // 3, 0, rows - rows // 4 - rows // 3], x.device)
    res = []
    for fused in (True, False):
        if fused:
            monkeypatch.delenv("GSVC_NO_FUSED_STE", raising=False)
        else:
            monkeypatch.setenv("GSVC_NO_FUSED_STE", "1")
        res.append(G._seg_ste(x, Q, seg, x_mean))
    a, b = res
    assert a.shape == b.shape == x.shape and not a.requires_grad
    assert torch.equal(a, b), ((a - b).abs().max().item(), (a != b).float().mean().item())
    # the clamp acted where the data asked for it
    q5 = Q[5].item() if per_row_q else Q
    assert abs(a[5].reshape(-1)[0].item()) < 3.0e4 or q5 * 15000 > 3.0e4
