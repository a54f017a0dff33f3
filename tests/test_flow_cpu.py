"""CPU tests of the optical-flow estimator: the NumPy restatement of tests/_flow_ref.py pins the algorithm and the convention of the
result (sign, x / y order, what the optical loss reads) independently of any kernel, and everything of csrc/flow.hip and gsvc_amd/flow.py
that runs before a launch (argument checks, the workspace query, the files ``save_flows`` writes)."""
import numpy as np
import pytest
import torch

from gsvc_amd import _lib, flow, io
from tests import _flow_ref as ref


# ---- quality: the algorithm finds a known shift ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ref.TABLE_SHAPES)
@pytest.mark.parametrize("shift", ref.SHIFTS)
def test_restatement_recovers_a_translation(shape, shift):
    """Mean endpoint error over ALL pixels, borders included, below 0.25 px (measured: 0.053 / 0.072 at 96 x 160, 0.125 / 0.162 at
    37 x 53, 0.132 / 0.179 at 18 x 34)."""
    a, b = ref.texture_pair(*shape, *shift)
    f = ref.estimate(a, b, np.float64)
    assert f.shape == (2,) + shape
    assert ref.epe(f, *shift) < 0.25, ref.epe(f, *shift)


@pytest.mark.parametrize("shape", ref.TABLE_SHAPES)
def test_restatement_of_a_still_pair_is_exactly_zero(shape):
    a, _ = ref.texture_pair(*shape, 0.0, 0.0)
    for dtype in (np.float64, np.float32):
        f = ref.estimate(a, a, dtype)
        assert f.dtype == dtype and not f.any()


def test_float32_restatement_is_within_the_bound():
    """The bound of the GPU test is 4 x the float32 restatement's distance from the float64 one on the GPU test's own cases, and at most
    1e-3 px: the restatement run in float32 stays inside it (the smaller shapes here; tools/bench_flow.py --f32-error prints all)."""
    assert set(ref.F32_ERRORS) == set(ref.CASES) and ref.F32_ERROR == max(ref.F32_ERRORS.values())
    assert ref.ESTIMATE_BOUND == min(4 * ref.F32_ERROR, 1e-3) and 0 < ref.F32_ERROR < 2.5e-4
    for case in ref.CASES[:4]:
        a, b = ref.case_inputs(case)
        got = np.abs(ref.estimate(a, b, np.float32).astype(np.float64) - ref.reference(case)).max()
        assert got <= ref.ESTIMATE_BOUND, (case, got)


def test_stages_by_hand():
    ramp = np.arange(12.0).reshape(3, 4)
    assert np.array_equal(ref.pool(np.arange(15.0).reshape(3, 5)), np.array([[(0 + 1 + 5 + 6) / 4, (2 + 3 + 7 + 8) / 4]]))          # odd row and column dropped
    assert np.allclose(ref.blur(np.full((5, 7), 0.3)), 0.3, rtol=0, atol=1e-16)
    impulse = np.zeros((9, 9))
    impulse[4, 4] = 256.0
    assert np.array_equal(ref.blur(impulse)[2:7, 2:7], np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]))
    corner = np.zeros((9, 9))
    corner[0, 0] = 256.0          # replicated borders: the corner sample is read 1 + 4 + 6 = 11 times per axis at (0, 0)
    assert ref.blur(corner)[0, 0] == 121.0
    assert ref.level_sizes(1080, 1920) == [(1080, 1920), (540, 960), (270, 480), (135, 240), (67, 120), (33, 60)]
    assert ref.level_sizes(18, 34) == [(18, 34), (9, 17)] and ref.level_sizes(37, 53) == [(37, 53), (18, 26), (9, 13)]
    assert ref.level_sizes(15, 40) == [(15, 40)]
    x, y = np.array([[1.25, -3.0, 9.0]]), np.array([[0.5, 0.0, 2.0]])
    assert np.allclose(ref.bilinear(ramp, x, y), [[1.25 + 0.5 * 4, 0.0, 11.0]])          # a ramp is reproduced; outside: clamped
    up = ref.upsample(np.array([[1.0, 3.0], [5.0, 7.0]]), 4, 4)
    assert np.allclose(up[0], [2.0, 3.0, 5.0, 6.0]) and np.allclose(up[:, 0], [2.0, 4.0, 8.0, 10.0])          # 2 x, half-pixel centres
    assert np.array_equal(ref.update(np.array([0.0, 0.0, 1.0]), np.array([2.5, -0.25, -3.0]), 1.0), [1.0, -0.25, 0.0])


def test_convention_is_what_the_optical_loss_reads():
    """A few points of the 96 x 160 pair, displaced by the flow as ``calc_optical_loss_one_frame`` reads it — the pixel is the rounded
    position, the field is indexed [x, y] after ``permute(2, 1, 0)``, the value is divided by ``scale`` — land within 0.25 px of where the
    true shift puts them."""
    H, W = 96, 160
    dx, dy = ref.SHIFTS[0]
    a, b = ref.texture_pair(H, W, dx, dy)
    field = torch.from_numpy(ref.estimate(a, b, np.float64).astype(np.float32))
    scale = max(H, W) / 2.0
    x_min, y_min = -W / 2 / scale, -H / 2 / scale
    pts_px = torch.tensor([[40.3, 30.6], [100.0, 50.0], [80.49, 70.2], [20.7, 60.1], [120.2, 20.8]])
    xy1 = pts_px / scale + torch.tensor([[x_min, y_min]])
    pix = ((xy1 - torch.tensor([[x_min, y_min]])) * scale).round().long()          # loss_utils.py: the pixel of frame 1
    uv = field.permute(2, 1, 0)[pix[:, 0], pix[:, 1], ...] / scale                   # loss_utils.py: flow[x, y] / scale
    moved_px = (xy1 + uv - torch.tensor([[x_min, y_min]])) * scale
    want = pts_px + torch.tensor([[dx, dy]])
    assert (moved_px - want).norm(dim=1).max() < 0.25, (moved_px - want)
    assert field.shape == (2, H, W) and abs(float(field[0].mean()) - dx) < 0.1 and abs(float(field[1].mean()) - dy) < 0.1


# ---- what runs before a launch -----------------------------------------------------------------------------------------------------
_NAMES = ("luma0", "luma1", "pitch", "n", "H", "W", "alpha", "warps", "iters", "min_side", "max_levels", "max_step", "out", "ws", "stream")
_OK = (1024, 4096, 40 * 48, 2, 40, 48, 0.02, 5, 30, 8, 6, 1.0, 8192, 65536, None)


def _but(**kw):
    return tuple(kw.get(n, v) for n, v in zip(_NAMES, _OK))


def test_estimate_entry_point_validates_on_the_host():
    L = _lib.lib()
    cases = [(_but(luma0=None), b"NULL"), (_but(luma1=None), b"NULL"), (_but(out=None), b"NULL"), (_but(ws=None), b"NULL"),
             (_but(n=0), b"n must be"), (_but(n=-3), b"n must be"), (_but(H=7), b"below min_side"), (_but(W=7), b"below min_side"),
             (_but(H=12, W=100, min_side=16), b"below min_side"), (_but(alpha=0.0), b"alpha must be positive"),
             (_but(alpha=-1.0), b"alpha must be positive"), (_but(warps=0), b"at least 1"), (_but(iters=0), b"at least 1"),
             (_but(max_levels=0), b"at least 1"), (_but(pitch=40 * 48 - 1), b"plane pitch"), (_but(ws=65536 + 8), b"16-byte aligned"),
             (_but(min_side=1), b"min_side must be at least 2"), (_but(max_step=0.0), b"max_step"), (_but(luma0=1026), b"4-byte aligned"),
             (_but(H=1, min_side=2), b"image size"), (_but(H=40000), b"image size")]
    for args, msg in cases:
        assert L.gsvc_flow_estimate(*args) == -1, args
        assert msg in L.gsvc_last_error(), (args, L.gsvc_last_error())


def _workspace_bytes(n, H, W, max_levels=6, min_side=8):
    """The layout the header describes: both pyramids, three flow fields and three coefficient planes at full size, each 256-byte padded."""
    pad = lambda v: -(-v // 256) * 256          # noqa: E731
    return sum(2 * pad(n * h * w * 4) for h, w in ref.level_sizes(H, W, min_side, max_levels)) + 3 * pad(n * 2 * H * W * 4) + 3 * pad(n * H * W * 4)


def test_workspace_query():
    L = _lib.lib()
    for n, H, W in ((1, 18, 34), (3, 37, 53), (16, 1080, 1920), (1, 8, 8)):
        assert L.gsvc_flow_workspace_bytes(n, H, W, 6, 8) == _workspace_bytes(n, H, W)
    assert L.gsvc_flow_workspace_bytes(2, 96, 160, 2, 8) == _workspace_bytes(2, 96, 160, 2, 8)
    assert L.gsvc_flow_workspace_bytes(16, 1080, 1920, 6, 8) < 48 * 16 * 1080 * 1920          # (flow.CHUNK's "about 47 bytes per pixel and pair")
    for bad in ((0, 40, 48, 6, 8), (1, 7, 48, 6, 8), (1, 40, 7, 6, 8), (1, 40, 48, 0, 8), (1, 40, 48, 6, 1), (1, 40000, 48, 6, 8), (70000, 40, 48, 6, 8)):
        assert L.gsvc_flow_workspace_bytes(*bad) < 0, bad
    assert L.gsvc_flow_solve_workspace_bytes(3, 37, 53) == 2 * (-(-3 * 2 * 37 * 53 * 4 // 256) * 256) and L.gsvc_flow_solve_workspace_bytes(0, 4, 4) < 0


def test_stage_entry_points_validate_on_the_host():
    L = _lib.lib()
    assert L.gsvc_flow_pyramid_step(None, 1, 8, 8, 0, 512, None) == -1 and b"NULL" in L.gsvc_last_error()
    assert L.gsvc_flow_pyramid_step(256, 1, 1, 8, 1, 512, None) == -1 and b"pooling needs" in L.gsvc_last_error()
    assert L.gsvc_flow_pyramid_step(256, 0, 8, 8, 0, 512, None) == -1 and b"n must be" in L.gsvc_last_error()
    warp_ok = (256, 512, 768, 1024, 1, 8, 8, None, None, 0, 0, 1280, 1536, 1792, None)
    assert L.gsvc_flow_warp(*(warp_ok[:2] + (None,) + warp_ok[3:])) == -1 and b"NULL" in L.gsvc_last_error()
    assert L.gsvc_flow_warp(*(warp_ok[:7] + (2048, None) + warp_ok[9:])) == -1 and b"go together" in L.gsvc_last_error()
    assert L.gsvc_flow_warp(*(warp_ok[:7] + (2048, 2304, 1, 4) + warp_ok[11:])) == -1 and b"coarse level" in L.gsvc_last_error()
    assert L.gsvc_flow_warp(*(warp_ok[:5] + (1, 8) + warp_ok[7:])) == -1 and b"image size" in L.gsvc_last_error()
    solve_ok = (256, 512, 768, 1024, 1280, None, None, 1, 8, 8, 0.02, 30, 1.0, 1536, 1792, 4096, None)
    assert L.gsvc_flow_solve(*(solve_ok[:11] + (0,) + solve_ok[12:])) == -1 and b"iters at least 1" in L.gsvc_last_error()
    assert L.gsvc_flow_solve(*(solve_ok[:5] + (2048, None) + solve_ok[7:])) == -1 and b"go together" in L.gsvc_last_error()
    assert L.gsvc_flow_solve(*(solve_ok[:13] + (256,) + solve_ok[14:])) == -1 and b"alias" in L.gsvc_last_error()
    assert L.gsvc_flow_solve(*(solve_ok[:15] + (4100, None))) == -1 and b"16-byte aligned" in L.gsvc_last_error()
    assert L.gsvc_flow_solve(*(solve_ok[:15] + (None, None))) == -1 and b"NULL" in L.gsvc_last_error()


def test_python_side_refuses_cpu_tensors_and_bad_shapes():
    x = torch.zeros(24, 32)
    with pytest.raises(_lib.GsvcError, match="CPU tensors"):
        flow.estimate_flow(x, x)
    with pytest.raises(_lib.GsvcError, match="CPU tensors"):
        flow.sequence_flow(torch.zeros(3, 24, 32))
    with pytest.raises(ValueError):
        flow.estimate_flow(np.zeros((24, 32)), x)
    with pytest.raises(TypeError):
        flow.FlowParams(sigma=1.0)
    p = flow.FlowParams()
    assert (p.alpha, p.warps, p.iters, p.min_side, p.max_levels, p.max_step) == tuple(ref.DEFAULTS[k] for k in ("alpha", "warps", "iters", "min_side", "max_levels", "max_step"))
    rgb = torch.rand(2, 3, 5, 7, dtype=torch.float64)
    assert torch.equal(flow.luma(rgb), 0.2126 * rgb[:, 0] + 0.7152 * rgb[:, 1] + 0.0722 * rgb[:, 2])
    assert np.allclose(ref.luma_of(rgb[0].numpy()), flow.luma(rgb[0]).numpy(), rtol=0, atol=1e-15)


def test_saved_flows_load_back_bit_for_bit(tmp_path):
    g = torch.Generator().manual_seed(3)
    fields = [torch.randn(2, 9, 13, generator=g) * 3 for _ in range(3)]
    fields[1][0, 0, 0], fields[1][1, 2, 3] = -0.0, 1e-42          # a signed zero and a denormal keep their bits
    paths = flow.save_flows(fields, tmp_path / "flows")
    assert [p.rsplit("/", 1)[1] for p in paths] == ["flow_00000.npy", "flow_00001.npy", "flow_00002.npy"]
    listed = sorted((tmp_path / "flows").iterdir())          # what VideoFileCube / FrameCubeDataset do with optical_flow_dir
    assert [str(p) for p in listed] == paths
    for p, f in zip(listed, fields):
        back = io.load_flow(p)
        assert back.dtype == torch.float32 and back.shape == f.shape
        assert torch.equal(back.view(torch.int32), f.view(torch.int32))
