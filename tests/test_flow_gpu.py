"""GPU tests of the optical-flow estimator (csrc/flow.hip, gsvc_amd/flow.py): every stage entry against its NumPy restatement alone
(tests/_flow_ref.py), the whole estimate against the float64 restatement within 4 x the float32 restatement's own error, batching and
determinism bit for bit, ``EstimatedFlowCube`` through the existing optical loss, and ``tools/fit_synthetic.py --estimate-flow``."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from gsvc_amd import _lib as lb
from gsvc_amd import flow
from tests import _flow_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRINT = bool(os.environ.get("GSVC_PRINT_ERRORS"))


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()          # (a copy: the shared inputs are read-only arrays)


def _report(what, got, bound):
    if PRINT:
        print(f"[flow] {what}: {got:.3e} (bound {bound:.3e})")


def _max_abs(t, want):
    return float(np.abs(t.cpu().numpy().astype(np.float64) - want).max())


@pytest.fixture(scope="module")
def stage_inputs():
    """Per shape, in float32 as the kernels get them: a texture pair (n = 2: both shifts), its blurred level, a smooth non-trivial flow."""
    out = {}
    for (H, W) in ref.SHAPES:
        pairs = [ref.texture_pair(H, W, *s) for s in ref.SHIFTS]
        a, b = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        # (reaches past every border: the outside ramp and the clamp of the bilinear read both act)
        u = np.stack([2.5 * np.sin(0.11 * xs + 0.07 * ys) + 1.5, -3.0 * np.cos(0.05 * xs - 0.13 * ys)]).astype(np.float32)
        v = np.stack([1.75 * np.cos(0.09 * xs) - 2.0, 2.25 * np.sin(0.08 * ys + 0.3) + 0.5]).astype(np.float32)
        out[(H, W)] = dict(a=a, b=b, u=u, v=v)
    return out


# ---- stages ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_pyramid_step(shape, stage_inputs):
    """blur and blur(pool(.)) of a batch of two planes: a few float32 ulps of a value of order 1."""
    H, W = shape
    a = stage_inputs[shape]["a"]
    L = lb.lib()
    src = _dev(a)
    st = lb.current_stream(src.device)
    full = torch.full((2, H, W), float("nan"), device="cuda")
    lb.check(L.gsvc_flow_pyramid_step(lb.ptr(src), 2, H, W, 0, lb.ptr(full), st), "gsvc_flow_pyramid_step")
    want = ref.blur(a.astype(np.float64))
    e0 = _max_abs(full, want)
    half = torch.full((2, H // 2, W // 2), float("nan"), device="cuda")
    lb.check(L.gsvc_flow_pyramid_step(lb.ptr(full), 2, H, W, 1, lb.ptr(half), st), "gsvc_flow_pyramid_step")
    e1 = _max_abs(half, ref.blur(ref.pool(full.cpu().numpy().astype(np.float64))))
    _report(f"pyramid {H}x{W} blur", e0, ref.PYRAMID_BOUND)
    _report(f"pyramid {H}x{W} pool + blur", e1, ref.PYRAMID_BOUND)
    assert e0 <= ref.PYRAMID_BOUND and e1 <= ref.PYRAMID_BOUND


def _warp(P0, P1, u, v, coarse=None):
    """gsvc_flow_warp on [n, h, w] arrays: (Ix, Iy, c, u0, v0) as device tensors; ``coarse`` = (cu, cv): u0, v0 are formed from them."""
    L = lb.lib()
    n, h, w = P0.shape
    tP0, tP1 = _dev(P0), _dev(P1)
    if coarse is None:
        tu, tv = _dev(u), _dev(v)
        cu = cv = None
        ch = cw = 0
    else:
        tu, tv = (torch.full((n, h, w), float("nan"), device="cuda") for _ in range(2))
        cu, cv = _dev(coarse[0]), _dev(coarse[1])
        ch, cw = coarse[0].shape[1:]
    Ix, Iy, c = (torch.full((n, h, w), float("nan"), device="cuda") for _ in range(3))
    lb.check(L.gsvc_flow_warp(lb.ptr(tP0), lb.ptr(tP1), lb.ptr(tu), lb.ptr(tv), n, h, w, lb.ptr(cu), lb.ptr(cv), ch, cw, lb.ptr(Ix), lb.ptr(Iy),
                              lb.ptr(c), lb.current_stream(tP0.device)), "gsvc_flow_warp")
    return Ix, Iy, c, tu, tv


# float32 against float64 on the same float32 inputs.  The warped position x + u0 rounds to half an ulp of 128 = 7.6e-6 px; the
# texture's slope is below 0.2 per px, so a sample of the warped picture is off by 1.5e-6 (+ three roundings of 6e-8 in the two lerps);
# a central difference of two such samples by as much, Ix and Iy by half of that plus the same from m; c = It - Ix u0 - Iy v0 with
# |u0|, |v0| <= 4.5 collects 1.5e-6 + 2 x 4.5 x 1.5e-6 = 1.5e-5.  Twice that; a wrong tap or border is 1e-2.
WARP_BOUND = 3e-5


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_warp_coefficients(shape, stage_inputs):
    H, W = shape
    s = stage_inputs[shape]
    P0, P1 = ref.blur(s["a"]), ref.blur(s["b"])          # float32 in, float32 out: what the kernel reads
    Ix, Iy, c, _, _ = _warp(P0, P1, s["u"], s["v"])
    for k in range(2):
        want = ref.warp_coefficients(P0[k].astype(np.float64), P1[k].astype(np.float64), s["u"][k].astype(np.float64), s["v"][k].astype(np.float64))
        for name, got, w64 in zip(("Ix", "Iy", "c"), (Ix, Iy, c), want):
            e = _max_abs(got[k], w64)
            _report(f"warp {H}x{W} pair {k} {name}", e, WARP_BOUND)
            assert e <= WARP_BOUND, (name, k, e)


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_warp_with_fused_upsampling(shape, stage_inputs):
    """The coarse flow (the level below: h // 2 x w // 2) is upsampled inside the pass: u0, v0 come out as the restatement's upsampling
    gives them in float32 — bit for bit, the positions and weights are exact — and the coefficients are those of the plain pass on them."""
    H, W = shape
    s = stage_inputs[shape]
    P0, P1 = ref.blur(s["a"]), ref.blur(s["b"])
    cu, cv = s["u"][:, :H // 2, :W // 2].copy(), s["v"][:, :H // 2, :W // 2].copy()
    Ix, Iy, c, u0, v0 = _warp(P0, P1, None, None, coarse=(cu, cv))
    want_u = np.stack([ref.upsample(cu[k], H, W) for k in range(2)])
    want_v = np.stack([ref.upsample(cv[k], H, W) for k in range(2)])
    assert want_u.dtype == np.float32
    assert np.array_equal(u0.cpu().numpy(), want_u) and np.array_equal(v0.cpu().numpy(), want_v)
    Ix2, Iy2, c2, _, _ = _warp(P0, P1, want_u, want_v)
    assert torch.equal(Ix, Ix2) and torch.equal(Iy, Iy2) and torch.equal(c, c2)


def _solve(U, V, Ix, Iy, c, iters, base=None, alpha=0.02, max_step=1.0):
    L = lb.lib()
    n, h, w = U.shape
    t = [_dev(x) for x in (U, V, Ix, Iy, c)]
    bu, bv = (_dev(base[0]), _dev(base[1])) if base is not None else (None, None)
    ou, ov = (torch.full((n, h, w), float("nan"), device="cuda") for _ in range(2))
    ws = torch.empty(int(L.gsvc_flow_solve_workspace_bytes(n, h, w)), dtype=torch.uint8, device="cuda")
    ws.fill_(0xFF)          # (NaN patterns: nothing of the workspace is relied on)
    lb.check(L.gsvc_flow_solve(*(lb.ptr(x) for x in t), lb.ptr(bu), lb.ptr(bv), n, h, w, alpha, iters, max_step, lb.ptr(ou), lb.ptr(ov),
                               lb.ptr(ws), lb.current_stream(ou.device)), "gsvc_flow_solve")
    return ou, ov


# float32 against float64 from the same float32 inputs.  A sweep is an average of four neighbours followed by a projection: it does not
# amplify what the previous sweep left, so the roundings of the sweeps at most add.  One sweep's own: three roundings of half an ulp of
# |Ix Ub + Iy Vb + c| < 4 (2^-23 each) times Ix den <= 1 / (2 alpha) = 25, 9e-6, and three of half an ulp of |U| <= 4.5 in the average,
# 7e-7: 1e-5 per sweep.  A wrong halo, ring or edge clamp is 1e-2 and more.
SOLVE_BOUND_PER_SWEEP = 1e-5


@pytest.mark.parametrize("iters", (1, ref.SOLVER_K, ref.SOLVER_K + 1, 30))
@pytest.mark.parametrize("shape", ref.SHAPES)
def test_solver_sweeps(shape, iters, stage_inputs):
    """``iters`` Jacobi sweeps from a given U, V and the coefficients of a warp, against the restatement's sweeps: 1 (no halo is used up),
    k (all of it), k + 1 (a second launch of one sweep) and 30 (the default; 8 launches on a tiled level, one on a level of one tile)."""
    H, W = shape
    s = stage_inputs[shape]
    P0, P1 = ref.blur(s["a"]), ref.blur(s["b"])
    Ix, Iy, c = (np.stack(x) for x in zip(*[ref.warp_coefficients(P0[k], P1[k], s["u"][k], s["v"][k]) for k in range(2)]))
    ou, ov = _solve(s["u"], s["v"], Ix, Iy, c, iters)
    for k in range(2):
        wu, wv = ref.solve(*(x[k].astype(np.float64) for x in (s["u"], s["v"], Ix, Iy, c)), 0.02, iters)
        e = max(_max_abs(ou[k], wu), _max_abs(ov[k], wv))
        _report(f"solve {H}x{W} iters {iters} pair {k}", e, iters * SOLVE_BOUND_PER_SWEEP)
        assert e <= iters * SOLVE_BOUND_PER_SWEEP, (k, e)
    if iters == ref.SOLVER_K + 1:
        # the clamped update is the epilogue of the last launch: from the launch's own U, V exactly
        bu, bv = s["u"] + np.float32(0.75), s["v"] - np.float32(0.5)
        cu, cv = _solve(s["u"], s["v"], Ix, Iy, c, iters, base=(bu, bv), max_step=0.5)
        assert np.array_equal(cu.cpu().numpy(), ref.update(bu, ou.cpu().numpy(), 0.5)) and np.array_equal(cv.cpu().numpy(), ref.update(bv, ov.cpu().numpy(), 0.5))
        assert float((cu - _dev(bu)).abs().max()) <= 0.5 + 1e-6 and float((cu - ou).abs().max()) > 0.1          # (the clamp did act)


def test_solver_sweeps_do_not_depend_on_the_blocking():
    """30 sweeps in launches of 4 = 30 launches' worth of single sweeps chained by hand: the same bits (Jacobi: the blocked form does the
    same operations on the same values)."""
    shape = ref.SHAPES[2]
    H, W = shape
    a, b = ref.texture_pair(H, W, *ref.SHIFTS[0])
    P0, P1 = ref.blur(a[None]), ref.blur(b[None])
    u = np.zeros((1, H, W), np.float32)
    Ix, Iy, c = (x[None] for x in ref.warp_coefficients(P0[0], P1[0], u[0], u[0]))
    ou, ov = _solve(u, u, Ix, Iy, c, 9)
    su, sv = u, u
    for _ in range(9):
        tu, tv = _solve(su, sv, Ix, Iy, c, 1)
        su, sv = tu.cpu().numpy(), tv.cpu().numpy()
    assert np.array_equal(ou.cpu().numpy(), su) and np.array_equal(ov.cpu().numpy(), sv)
    assert float(np.abs(su).max()) > 0.1


# ---- whole -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def estimates():
    """The kernel path's estimate of every case, once."""
    out = {}
    for case in ref.CASES:
        a, b = ref.case_inputs(case)
        out[case] = flow.estimate_flow(_dev(a), _dev(b))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", ref.CASES, ids=[str(c) for c in ref.CASES])
def test_estimate_against_the_float64_restatement(case, estimates):
    """Max |kernel - float64 restatement| in px over both components and all pixels within ESTIMATE_BOUND = 4 x the float32
    restatement's distance from the float64 one on these same inputs (6.2e-4 px; tests/_flow_ref.py)."""
    got = estimates[case]
    want = ref.reference(case)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    e = _max_abs(got, want)
    _report(f"estimate {case}", e, ref.ESTIMATE_BOUND)
    assert e <= ref.ESTIMATE_BOUND, (case, e)
    if case != "cube":
        assert ref.epe(got.cpu().numpy().astype(np.float64), case[2], case[3]) < 0.25


def test_batching_determinism_and_pitch(estimates):
    """A batch of 3 pairs = three calls of 1; two runs agree; a plane pitch above H W with guard values between the planes, a dirty
    workspace and bytes beyond flow_out change nothing — all bit for bit."""
    H, W = ref.SHAPES[1]
    cases = [(H, W) + s for s in ref.SHIFTS] + [(H, W) + ref.SHIFTS[0]]
    a = torch.stack([_dev(ref.case_inputs(c)[0]) for c in cases])
    b = torch.stack([_dev(ref.case_inputs(c)[1]) for c in cases])
    b[2] = a[2]          # (the third pair is still: exactly zero flow)
    got = flow.estimate_flow(a.unsqueeze(1), b.unsqueeze(1))
    assert tuple(got.shape) == (3, 2, H, W)
    assert torch.equal(got[0], estimates[cases[0]]) and torch.equal(got[1], estimates[cases[1]])
    assert not got[2].any()
    assert torch.equal(got, flow.estimate_flow(a.unsqueeze(1), b.unsqueeze(1)))
    # the C entry point with a pitch of H W + 37 floats, NaN guards, a workspace and an output buffer full of NaN patterns
    L = lb.lib()
    pitch = H * W + 37
    la, lb_ = (torch.full((3, pitch), float("nan"), device="cuda") for _ in range(2))
    la[:, :H * W], lb_[:, :H * W] = a.reshape(3, -1), b.reshape(3, -1)
    out = torch.full((3 * 2 * H * W + 64,), float("nan"), device="cuda")
    ws = torch.empty(int(L.gsvc_flow_workspace_bytes(3, H, W, 6, 8)), dtype=torch.uint8, device="cuda")
    ws.fill_(0xFF)
    lb.check(L.gsvc_flow_estimate(lb.ptr(la), lb.ptr(lb_), pitch, 3, H, W, 0.02, 5, 30, 8, 6, 1.0, lb.ptr(out), lb.ptr(ws),
                                  lb.current_stream(out.device)), "gsvc_flow_estimate")
    assert torch.equal(out[:3 * 2 * H * W].view(3, 2, H, W), got)
    assert bool(torch.isnan(out[3 * 2 * H * W:]).all()) and bool(torch.isnan(la[:, H * W:]).all())


def test_sequence_reads_the_frames_where_they_lie():
    """T frames, pair k = frames k and k + 1 through one call with luma1 = luma0 + pitch: the pairs' own estimates, bit for bit; RGB
    pictures give the estimate of their lumas."""
    H, W = ref.SHAPES[0]
    frames = torch.stack([_dev(ref.texture_pair(H, W, 0.9 * k, -0.6 * k)[1]) for k in range(4)])
    seq = flow.sequence_flow(frames)
    assert tuple(seq.shape) == (3, 2, H, W)
    for k in range(3):
        assert torch.equal(seq[k], flow.estimate_flow(frames[k], frames[k + 1]))
    rgb = torch.stack([frames[:3] * 0.9, frames[:3] * 0.5 + 0.2, frames[:3]], dim=1)          # [n, 3, H, W]
    assert torch.equal(flow.estimate_flow(rgb[:2], rgb[1:]), flow.estimate_flow(flow.luma(rgb[:2]).unsqueeze(1), flow.luma(rgb[1:]).unsqueeze(1)))
    assert torch.equal(flow.estimate_flow(rgb[0], rgb[1]), flow.estimate_flow(rgb[:2], rgb[1:])[0])
    few = flow.estimate_flow(frames[0], frames[1], warps=2, iters=7, max_levels=1)
    want = ref.estimate(frames[0].cpu().numpy(), frames[1].cpu().numpy(), np.float64, warps=2, iters=7, max_levels=1)
    assert _max_abs(few, want) <= ref.ESTIMATE_BOUND


# ---- the cube and the tool ---------------------------------------------------------------------------------------------------------
def test_estimated_flow_cube():
    from types import SimpleNamespace

    from gsvc_amd import loss_utils as LU
    from gsvc_amd.frame import SyntheticFrameCube
    H, W, T = 48, 80, 4
    cube = SyntheticFrameCube(H, W, T, device="cuda")
    est = flow.EstimatedFlowCube(cube)
    assert len(est) == T and est.len_z_frames == T and est.scale == cube.scale and est.x_min == cube.x_min and est.height == H
    assert tuple(est.flows.shape) == (T - 1, 2, H, W) and est.flows.dtype == torch.float32 and est.flows.is_cuda
    for i in range(T - 1):
        f = est.get_optical_flow(i)
        assert tuple(f.shape) == (2, H, W)
        # the cube hands its pictures out transposed [3, W, H]; the estimator is given [H, W]
        assert torch.equal(f, flow.estimate_flow(cube[i].image.permute(0, 2, 1), cube[i + 1].image.permute(0, 2, 1)))
    fr, want = est[1], cube[1]
    assert fr.image_id == want.image_id and fr.z == want.z and torch.equal(fr.image, want.image) and torch.equal(fr.view_matrix, want.view_matrix)
    assert est.get_dummy_frame(2).image is None and est.get_z_frame(2).image_id == 2
    # the estimate is nearer to the cube's analytic field than no flow is
    epe = float((est.get_optical_flow(1) - cube.get_optical_flow(1)).square().sum(0).sqrt().mean())
    assert epe < float(cube.get_optical_flow(1).square().sum(0).sqrt().mean())
    # one evaluation of the optical loss through the existing path (un-compacted renders, csrc/losses.hip)
    K, A = 4, 900
    scale = est.scale
    x_min, y_min = est.x_min, est.y_min

    def fake_render(seed):
        gg = torch.Generator().manual_seed(seed)
        vis_mask = torch.rand(A, generator=gg) < 0.6
        vis = vis_mask.nonzero().squeeze(1).cuda()
        rows = vis.shape[0]
        world = torch.stack([(torch.rand(rows * K, generator=gg) * 1.2 - 0.6) * (-2 * x_min), (torch.rand(rows * K, generator=gg) * 1.2 - 0.6) * (-2 * y_min),
                             torch.rand(rows * K, generator=gg)], 1).cuda().requires_grad_(True)
        m = (torch.rand(rows * K, generator=gg) < 0.7).cuda()
        gsd = SimpleNamespace(world_xyz=world, mask=m)
        return SimpleNamespace(visible_mask=vis_mask.cuda(), visible_index=vis, generated_gaussians=gsd, dense=True), world

    rs = [fake_render(s) for s in (11, 12, 13, 14)]
    loss = LU.calc_optical_loss(rs[0][0], rs[1][0], rs[2][0], rs[3][0], est.get_optical_flow(1), x_min, y_min, scale, W, H, K)
    loss.backward()
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0
    for _, world in rs:
        assert world.grad is not None and bool(torch.isfinite(world.grad).all())
    assert any(float(world.grad.abs().max()) > 0 for _, world in rs)


@pytest.mark.parametrize("resident", ("float", "u8"))
def test_estimated_flow_of_a_video_file(tmp_path, resident):
    """A video file holds no flow; wrapped, it answers with the estimate of its own pictures."""
    from gsvc_amd.frames_in import VideoFileCube
    H, W, T = 24, 40, 3
    frames = np.stack([np.repeat((ref.texture_pair(H, W, 1.5 * k, -0.8 * k)[1] * 255).round().astype(np.uint8)[..., None], 3, axis=2) for k in range(T)])
    (tmp_path / "v.rgb").write_bytes(frames.tobytes())
    cube = VideoFileCube(tmp_path / "v.rgb", W=W, H=H, resident=resident)
    with pytest.raises(RuntimeError, match="holds no optical flow"):
        cube.get_optical_flow(0)
    est = flow.EstimatedFlowCube(cube, warps=3)
    assert est.flow_params.warps == 3 and est.fmt is cube.fmt and est.resident == resident and len(est) == T
    for i in range(T - 1):
        want = flow.estimate_flow(cube[i].image.permute(0, 2, 1), cube[i + 1].image.permute(0, 2, 1), warps=3)
        assert torch.equal(est.get_optical_flow(i), want) and tuple(want.shape) == (2, H, W)
    assert abs(float(est.get_optical_flow(0)[0].mean()) - 1.5) < 0.3 and abs(float(est.get_optical_flow(0)[1].mean()) + 0.8) < 0.3
    paths = est.save_flows(tmp_path / "flows")
    again = VideoFileCube(tmp_path / "v.rgb", optical_flow_dir=tmp_path / "flows", W=W, H=H, resident=resident)
    assert len(paths) == T - 1 and torch.equal(again.get_optical_flow(1), est.get_optical_flow(1))


def test_fit_tool_with_estimated_flow(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fit_synthetic
    out = tmp_path / "rd.json"
    # the toy setting of tests/test_fit_tool_gpu.py, at which the tool's own identities hold (measured with the estimated flow: decoded
    # against quantised model 0.003 dB where the tool allows 0.01; over 2 evaluated frames instead of 6 it was 0.012)
    fit_synthetic.main(["--estimate-flow", "--steps", "240", "--height", "272", "--width", "480", "--frames", "24", "--anchors", "12000", "--eval-frames", "6",
                        "--slab-frames", "8", "--densify-grad-threshold", "2e-5", "--payload-tol", "0.12", "--json", str(out)])
    log = json.loads(out.read_text())
    assert log["flow"]["source"] == "estimated" and log["flow"]["optical_lambda"] > 0 and log["flow"]["pairs"] == 23
    assert log["flow"]["params"] == ref.DEFAULTS
    # (recorded, not bounded: the cube's analytic field blends the blobs' velocities over the whole frame, also where the picture is its
    # still background; at this size the estimate is 1.17 px from it and zero flow 1.11 px)
    assert log["flow"]["mean_epe_vs_analytic_px"] > 0 and log["flow"]["mean_analytic_magnitude_px"] > 0
    assert len(log["phases"]) == 4 and log["bpp"] > 0
