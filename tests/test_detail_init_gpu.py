"""GPU tests of the content-adaptive initial anchors (csrc/detail.hip, gsvc_amd/detail.py): the detail map and the
sampler are bit-equal to the integer statement of tests/_detail_ref.py at the shapes where the kernels can go wrong (a picture smaller than
a cell, partial cells, more than one tile each way, both load paths, every cell size and sample width, the chunk overlap); the points
land where the picture has detail, also when they are RENDERED; ``cube_detail`` gives one map for every way of holding a video; the two
initialisations of ``new_fit`` are what they say; the encoder tool's file decodes in a fresh process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gsvc_amd import _lib, detail
from gsvc_amd.frames_out import LAYOUTS, FrameFormat, Y4MWriter, frame_bytes
from tests import _detail_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GUARD = 64          # sentinel elements in front of and behind an output


def _guarded(count, dtype, fill):
    """A tensor of ``count`` elements pre-filled with garbage, with GUARD sentinel elements (all bits set) on either side."""
    whole = torch.full((count + 2 * GUARD,), -1, dtype=torch.int32, device=DEV)
    inner = whole[GUARD:GUARD + count].view(dtype)          # (both element types used here have four bytes)
    inner.fill_(fill)
    return whole, inner


def _guards_intact(whole, count):
    bits = whole.view(torch.int32)
    return bool((bits[:GUARD] == -1).all()) and bool((bits[GUARD + count:] == -1).all())


def _detail_raw(view, stride, n, n_out, H, W, fmt, cell):
    """gsvc_frames_detail on the frames that start at ``view`` (a uint8 CUDA tensor; its first element is the base), into a guarded,
    garbage-filled output -> uint32 numpy ``[n_out, Hc, Wc]``."""
    Hc, Wc = detail.map_shape(H, W, cell)
    count = n_out * Hc * Wc
    whole, out = _guarded(count, torch.int32, 0x5A5A5A5A)
    _lib.check(_lib.lib().gsvc_frames_detail(view.data_ptr(), stride, n, n_out, H, W, LAYOUTS[fmt.layout], fmt.depth, cell, out.data_ptr(),
                                             _lib.current_stream(torch.device(DEV))), "gsvc_frames_detail")
    assert _guards_intact(whole, count), (H, W, n, n_out, cell)
    return out.cpu().numpy().view(np.uint32).reshape(n_out, Hc, Wc)


def _random_frames(rng, n, H, W, fmt):
    nbytes = frame_bytes(H, W, fmt)
    if fmt.depth > 8:
        top = 65536 if fmt.depth == 16 else 1 << fmt.depth
        return rng.integers(0, top, (n, nbytes // 2), dtype=np.uint16).astype("<u2").view(np.uint8).reshape(n, nbytes)
    return rng.integers(0, 256, (n, nbytes), dtype=np.uint8)


def _placed(frames, stride, offset):
    """The frames laid out ``stride`` bytes apart from byte ``offset`` of a 16-byte aligned buffer whose other bytes are 0xFF."""
    n, nbytes = frames.shape
    host = np.full(offset + n * stride + 16, 0xFF, np.uint8)
    for k in range(n):
        host[offset + k * stride:offset + k * stride + nbytes] = frames[k]
    buf = torch.from_numpy(host).to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf[offset:]


SIZES = [(1, 1), (2, 2), (5, 7), (6, 10), (18, 34), (96, 64), (64, 96), (160, 300), (300, 160)]          # H, W


@pytest.mark.parametrize("depth", [8, 10, 16])
def test_map_is_the_reference_bit_for_bit(depth):
    """Every size, cell and frame count, at four placements: tight at a 16-byte aligned base (the wide path where W allows it), the base
    moved by one sample (edge path), the stride padded by 16 bytes (wide) and by one sample (edge), 0xFF between the frames."""
    rng = np.random.default_rng(100 + depth)
    bps = 2 if depth > 8 else 1
    for H, W in SIZES:
        layouts = ["yuv444p"] if (H % 2 or W % 2) else (["yuv420p", "yuv444p"] if (H, W) == (18, 34) else ["yuv420p"])
        for layout in layouts:
            fmt = FrameFormat(layout, depth=depth)
            nbytes = frame_bytes(H, W, fmt)
            frames = _random_frames(rng, 3, H, W, fmt)
            luma = ref.luma_of(frames, H, W, depth)
            for n, n_out in ((1, 1), (2, 2), (3, 1), (3, 2), (3, 3)):
                for cell in (4, 8, 16):
                    want = ref.detail_map_ref(luma[:n], cell, n_out)
                    assert want.max() < 2 ** 32
                    for stride, offset in ((nbytes + (-nbytes) % 16, 0), (nbytes + (-nbytes) % 16, bps), (nbytes + (-nbytes) % 16 + 16, 0),
                                           (nbytes + bps, 0), (nbytes, 0)):
                        got = _detail_raw(_placed(frames[:n], stride, offset), stride, n, n_out, H, W, fmt, cell)
                        assert np.array_equal(got.astype(np.int64), want), (H, W, layout, n, n_out, cell, stride, offset)


def test_wide_and_edge_paths_agree_and_the_wrapper_is_the_entry():
    """One picture of more than one tile each way, W a multiple of 16: the aligned placement takes the vector loads, the moved one the
    sample loads; the bits are the same, and ``luma_detail`` returns them."""
    rng = np.random.default_rng(5)
    H, W = 70, 272
    for depth in (8, 10):
        fmt = FrameFormat("yuv420p", depth=depth)
        nbytes, bps = frame_bytes(H, W, fmt), 2 if depth > 8 else 1
        assert nbytes % 16 == 0
        frames = _random_frames(rng, 3, H, W, fmt)
        for cell in (4, 8, 16):
            wide = _detail_raw(_placed(frames, nbytes, 0), nbytes, 3, 3, H, W, fmt, cell)
            edge = _detail_raw(_placed(frames, nbytes, bps), nbytes, 3, 3, H, W, fmt, cell)
            assert np.array_equal(wide, edge) and wide.any()
            assert np.array_equal(wide.astype(np.int64), ref.detail_map_ref(ref.luma_of(frames, H, W, depth), cell))
            m = detail.luma_detail(torch.from_numpy(frames).to(DEV), H, W, fmt, cell)
            assert m.dtype == torch.uint32 and np.array_equal(m.cpu().numpy(), wide)
            m2 = detail.luma_detail(torch.from_numpy(frames).to(DEV), H, W, fmt, cell, n_out=2)
            assert np.array_equal(m2.cpu().numpy(), wide[:2])


def test_extreme_codes_reach_the_largest_sum_exactly():
    """0 / 65535 boards of 2 x 2 squares, in opposite phase in the two frames: every central difference and the temporal difference
    are 65535, so an inner cell of 16 x 16 holds 4 * 65535 * 256, the largest value there is."""
    H, W = 64, 160
    fmt = FrameFormat("yuv444p", depth=16)
    ys, xs = np.mgrid[0:H, 0:W]
    board = (((ys >> 1) + (xs >> 1)) & 1).astype(np.uint16) * 65535
    frames = np.zeros((2, frame_bytes(H, W, fmt) // 2), "<u2")
    frames[0, :H * W], frames[1, :H * W] = board.reshape(-1), (65535 - board).reshape(-1)
    frames = frames.view(np.uint8).reshape(2, -1)
    want = ref.detail_map_ref(ref.luma_of(frames, H, W, 16), 16)
    assert want[0, 1, 1] == 4 * 65535 * 256 and want.max() == 4 * 65535 * 256
    for offset in (0, 2):
        got = _detail_raw(_placed(frames, frames.shape[1], offset), frames.shape[1], 2, 2, H, W, fmt, 16)
        assert np.array_equal(got.astype(np.int64), want)


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------
def _sample_raw(dmap, H, W, cell, N, seed, mix24):
    """gsvc_detail_sample on an integer map (numpy ``[T, Hc, Wc]``), guarded outputs -> (float32 ``[N, 3]``, int32 ``[N]``)."""
    cdf = torch.cumsum(torch.from_numpy(np.asarray(dmap, np.int64).reshape(-1)).to(DEV), 0)
    pw, points = _guarded(3 * N, torch.float32, 12345.0)
    cw, cell_of = _guarded(N, torch.int32, 0x5A5A5A5A)
    _lib.check(_lib.lib().gsvc_detail_sample(cdf.data_ptr(), int(cdf.shape[0]), int(dmap.shape[0]), H, W, cell, N, seed, mix24, points.data_ptr(),
                                             cell_of.data_ptr(), _lib.current_stream(torch.device(DEV))), "gsvc_detail_sample")
    assert _guards_intact(pw, 3 * N) and _guards_intact(cw, N)
    return points.cpu().numpy().reshape(N, 3), cell_of.cpu().numpy()


@pytest.fixture(scope="module")
def sampler_map():
    rng = np.random.default_rng(11)
    m = rng.integers(0, 2 ** 32, (4, 6, 8), dtype=np.uint64).astype(np.int64)
    m[rng.random(m.shape) < 0.4] = 0
    m[0, 0, 0] = m[3, 5, 7] = 0          # the first and the last cell cannot be drawn from the map
    return m


@pytest.mark.parametrize("seed", [0, 1234])
@pytest.mark.parametrize("mix", [0.0, 0.25, 1.0])
def test_sampler_is_the_reference_exactly(sampler_map, seed, mix):
    H, W, cell, N = 48, 64, 8, 4096
    mix24 = detail.mix24_of(mix)
    want_p, want_c = ref.sample_ref(sampler_map, H, W, cell, N, seed, mix24)
    got_p, got_c = _sample_raw(sampler_map, H, W, cell, N, seed, mix24)
    assert np.array_equal(got_c, want_c)
    assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
    if mix == 0.0:
        assert (sampler_map.reshape(-1)[got_c] > 0).all()
    # the wrapper: the same draw from the uint32 map, and the total
    dmap = torch.from_numpy(sampler_map.astype(np.uint32)).to(DEV)
    p, c, total = detail.sample_points(dmap, H, W, cell, N, mix, seed)
    assert np.array_equal(p.cpu().numpy().view(np.uint32), want_p.view(np.uint32)) and np.array_equal(c.cpu().numpy(), want_c)
    assert int(total) == int(sampler_map.sum())


def test_sampler_on_a_map_of_zeros_and_on_partial_cells():
    zero = np.zeros((4, 6, 8), np.int64)
    want_p, want_c = ref.sample_ref(zero, 48, 64, 8, 1000, 7, 0)
    got_p, got_c = _sample_raw(zero, 48, 64, 8, 1000, 7, 0)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
    H, W = 50, 70          # 7 x 9 cells of 8: the last row is 2 pixels high, the last column 6 wide
    rng = np.random.default_rng(12)
    m = rng.integers(1, 1000, (2, 7, 9)).astype(np.int64)
    m[:, 6, :] *= 50
    m[:, :, 8] *= 50          # most points fall into the partial cells
    for mix24 in (0, 1 << 22):
        want_p, want_c = ref.sample_ref(m, H, W, 8, 2000, 3, mix24)
        got_p, got_c = _sample_raw(m, H, W, 8, 2000, 3, mix24)
        assert np.array_equal(got_c, want_c) and np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
        assert got_p[:, 0].max() < W and got_p[:, 1].max() < H and got_p[:, :2].min() >= 0
        assert got_p[:, 2].min() >= -0.5 and got_p[:, 2].max() < 1.5
    assert np.mean(want_c % 63 >= 54) > 0.3


# ---- placement ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def quadrant(tmp_path_factory):
    """The placement clip as a file, its cube and its map at cell 8."""
    from gsvc_amd.frames_in import VideoFileCube
    H, W = 48, 64
    fmt = FrameFormat("yuv420p")
    frames = ref.quadrant_clip()
    path = str(tmp_path_factory.mktemp("detail") / "quadrant.y4m")
    with Y4MWriter(path, W, H, (25, 1), fmt) as sink:
        for fr in frames:
            sink.write(fr)
    cube = VideoFileCube(path, device=DEV, resident="u8")
    dmap = detail.cube_detail(cube, 8)
    assert np.array_equal(dmap.cpu().numpy().astype(np.int64), ref.detail_map_ref(ref.luma_of(frames, H, W, 8), 8))
    return {"cube": cube, "map": dmap, "H": H, "W": W}


def test_points_go_where_the_detail_is(quadrant):
    H, W = quadrant["H"], quadrant["W"]

    def share(mix):
        p = detail.sample_points(quadrant["map"], H, W, 8, 4096, mix, 0)[0].cpu().numpy()
        return float(np.mean((p[:, 0] < W / 2) & (p[:, 1] < H / 2)))
    assert share(0.25) >= 0.78          # expectation 0.8125; the reference's draw gives 0.807 (tests/test_detail_init_cpu.py)
    assert share(0.0) == 1.0
    assert 0.22 <= share(1.0) <= 0.28
    # the world coordinates: inside the pictures and the clip, no bleed
    cube = quadrant["cube"]
    pts, total = detail.detail_points(cube, 4096, 8, 0.25, 0)
    assert pts.dtype == np.float64 and pts.shape == (4096, 3) and total == int(quadrant["map"].cpu().numpy().astype(np.int64).sum())
    assert (pts[:, 0] >= cube.x_min).all() and (pts[:, 0] < -cube.x_min).all() and (pts[:, 1] >= cube.y_min).all() and (pts[:, 1] < -cube.y_min).all()
    half = 0.5 / cube.scale          # frame t's camera sits at z_min + t / scale; its points lie within half a frame of it
    assert (pts[:, 2] >= cube.z_min - half).all() and (pts[:, 2] < -cube.z_min - half).all()
    assert np.mean((pts[:, 0] < 0) & (pts[:, 1] < 0)) >= 0.78


def test_orientation_by_rendering(quadrant):
    """The points of frame 1 (mix 0) as small opaque white Gaussians, rendered by the project's rasterizer through the camera of
    ``cube.get_z_frame(1)`` on black: the light must be in the top-left quadrant of the picture as the file stores it."""
    from gsvc_amd import rasterizer
    cube, H, W = quadrant["cube"], quadrant["H"], quadrant["W"]
    p, c, _ = detail.sample_points(quadrant["map"], H, W, 8, 4096, 0.0, 0)
    keep = (c // (6 * 8) == 1).cpu().numpy()
    assert keep.sum() > 500
    world = torch.from_numpy(detail.to_world(p.cpu().numpy()[keep], cube)).float().to(DEV)
    fr = cube.get_z_frame(1, load_image=False)
    n = world.shape[0]
    rs = rasterizer.GaussianRasterizationSettings(
        image_height=H, image_width=W, x_min=fr.x_min, y_min=fr.y_min, scale=fr.scale, threshold=1.0 / cube.scale, bg=torch.zeros(3),
        scale_modifier=1.0, viewmatrix=fr.view_matrix.permute(1, 0), sh_degree=0, campos=fr.cam_pos, prefiltered=False, debug=False)
    image, radii, _ = rasterizer.GaussianRasterizer(raster_settings=rs)(
        means3D=world, means2D=torch.zeros_like(world), shs=None, colors_precomp=torch.ones((n, 3), device=DEV),
        opacities=torch.full((n, 1), 0.99, device=DEV), scales=torch.full((n, 3), 0.7 / cube.scale, device=DEV),
        rotations=torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=DEV).repeat(n, 1), cov3D_precomp=None)
    image = image.detach()
    assert tuple(image.shape) == (3, H, W) and float(image.sum()) > 100.0 and int((radii > 0).sum()) > 500
    assert float(image[:, :H // 2, :W // 2].sum()) >= 0.9 * float(image.sum())


# ---- one map for every way of holding a video -------------------------------------------------------------------------------------------
def _write_clip(path, frames, H, W, fmt):
    with Y4MWriter(path, W, H, (25, 1), fmt) as sink:
        for fr in frames:
            sink.write(fr)


@pytest.mark.parametrize("T,depth", [(17, 8), (33, 10), (5, 8)])
def test_cube_detail_is_the_same_in_either_residency_and_range(tmp_path, T, depth):
    from gsvc_amd.frames_in import VideoFileCube
    H, W = 16, 24
    fmt = FrameFormat("yuv420p", depth=depth)
    frames = _random_frames(np.random.default_rng(T), T, H, W, fmt)
    if depth == 10:
        frames = (frames.view("<u2") & 1023).view(np.uint8)
    path = str(tmp_path / "clip.y4m")
    _write_clip(path, frames, H, W, fmt)
    want = ref.detail_map_ref(ref.luma_of(frames, H, W, depth), 8)
    for resident in ("u8", "float"):
        cube = VideoFileCube(path, device=DEV, resident=resident)
        assert np.array_equal(detail.cube_detail(cube, 8).cpu().numpy().astype(np.int64), want), resident
        assert np.array_equal(cube.luma_detail(8).cpu().numpy().astype(np.int64), want), resident
    # a range of the file against a file cut to that range: the last frame looks back, never across the cut
    first, stop = 2, T - 1
    cut = str(tmp_path / "cut.y4m")
    _write_clip(cut, frames[first:stop], H, W, fmt)
    want_cut = ref.detail_map_ref(ref.luma_of(frames[first:stop], H, W, depth), 8)
    assert not np.array_equal(want_cut[-1], want[stop - 1])
    for resident in ("u8", "float"):
        ranged = detail.cube_detail(VideoFileCube(path, device=DEV, resident=resident, frame_range=(first, stop)), 8).cpu().numpy()
        whole = detail.cube_detail(VideoFileCube(cut, device=DEV, resident=resident), 8).cpu().numpy()
        assert np.array_equal(ranged, whole) and np.array_equal(ranged.astype(np.int64), want_cut), resident


def test_cube_detail_through_the_flow_cube_and_of_float_cubes(quadrant):
    from gsvc_amd.flow import EstimatedFlowCube
    from gsvc_amd.frame import HostResidentCube, SyntheticFrameCube
    from gsvc_amd.frames_out import frames_to_u8
    wrapped = EstimatedFlowCube(quadrant["cube"], device=DEV)
    assert torch.equal(detail.cube_detail(wrapped, 8), quadrant["map"]) and torch.equal(wrapped.luma_detail(8), quadrant["map"])
    # a cube of float pictures: 16-bit full-range 4:4:4 codes of them, T = 19 in two overlapped windows
    H, W, T = 20, 36, 19
    cube = SyntheticFrameCube(H, W, T, seed=3, device=DEV).materialize()
    codes = FrameFormat("yuv444p", "bt709", "full", depth=16)
    buf = frames_to_u8([cube._image(t) for t in range(T)], codes).cpu().numpy()
    want = ref.detail_map_ref(ref.luma_of(buf, H, W, 16), 4)
    got = detail.cube_detail(cube, 4)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want) and want.any()
    assert torch.equal(detail.cube_detail(EstimatedFlowCube(cube, device=DEV), 4), got)
    assert torch.equal(detail.cube_detail(HostResidentCube(cube, DEV), 4), got)


# ---- the two initialisations of a fit --------------------------------------------------------------------------------------------------
def _fit_setup(init, anchors=3000, **kw):
    from gsvc_amd.arguments import cfg_20240919
    from gsvc_amd.fit_setup import configure_fit, new_fit
    from gsvc_amd.frame import SyntheticFrameCube
    dev = torch.device(DEV)
    mp_, opt, pipe = cfg_20240919()
    cube = SyntheticFrameCube(48, 64, 8, seed=1234, device=dev).materialize()
    configure_fit(mp_, opt, cube, 60, 0.004, 8.0, 2e-5)
    pc, trainer = new_fit(cube, mp_, opt, pipe, anchors, dev, init=init, **kw)
    trainer.close()
    return pc, cube, mp_


def test_detail_init_twice_gives_equal_anchors():
    a, cube, _ = _fit_setup("detail")
    b, _, _ = _fit_setup("detail")
    assert a._anchor.shape[0] > 100 and torch.equal(a._anchor, b._anchor) and torch.equal(a._scaling, b._scaling)
    p = a._anchor.detach().cpu().numpy()          # (a voxel's centre may lie half a voxel outside)
    lim = -np.array([cube.x_min, cube.y_min, cube.z_min - 0.5 / cube.scale]) + a.voxel_size          # (z: half a frame around a camera)
    assert (np.abs(p) <= lim).all()
    c, _, _ = _fit_setup("detail", init_cell=16, init_mix=1.0)
    assert not (c._anchor.shape == a._anchor.shape and torch.equal(c._anchor, a._anchor))


def test_uniform_init_is_the_parent_commits():
    """``init="uniform"`` (and no ``init`` at all) gives the anchors of the draw as it was: ``default_rng(0).uniform`` over the cube with
    the 10 % bleed, pushed through ``create_from_points`` by hand."""
    from gsvc_amd.model import GaussianModel
    from gsvc_amd.arguments import cfg_20240919
    from gsvc_amd.fit_setup import configure_fit, new_fit
    from gsvc_amd.frame import SyntheticFrameCube
    a, cube, mp_ = _fit_setup("uniform")
    torch.manual_seed(0)
    np.random.seed(0)
    pc = GaussianModel(mp_, mp_.anchor_feature_dim, mp_.n_offsets, mp_.voxel_size, mp_.update_depth, mp_.update_init_factor,
                       mp_.update_hierarchy_factor, mp_.use_feat_bank, n_features_per_level=mp_.grid_feature_dim,
                       log2_hashmap_size=mp_.log2, log2_hashmap_size_2D=mp_.log2_2D, device=torch.device(DEV))
    lim = np.array([cube.x_min, cube.y_min, cube.z_min]) * 1.1
    pc.create_from_points(np.random.default_rng(0).uniform(lim, -lim, (3000, 3)), spatial_lr_scale=1.0)
    assert torch.equal(a._anchor, pc._anchor) and torch.equal(a._scaling, pc._scaling)
    dev = torch.device(DEV)          # the default argument is that path
    mp2, opt2, pipe2 = cfg_20240919()
    cube2 = SyntheticFrameCube(48, 64, 8, seed=1234, device=dev).materialize()
    configure_fit(mp2, opt2, cube2, 60, 0.004, 8.0, 2e-5)
    b, trainer = new_fit(cube2, mp2, opt2, pipe2, 3000, dev)
    trainer.close()
    assert torch.equal(a._anchor, b._anchor)


def test_encode_tool_with_detail_init_then_decode_tool_in_another_process(tmp_path):
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import frames_to_u8
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gsvc_encode
    H, W, T = 48, 64, 8
    fmt = FrameFormat("yuv420p")
    cube = SyntheticFrameCube(H, W, T, seed=7, device="cuda")
    clip, out, coded = str(tmp_path / "clip.y4m"), str(tmp_path / "out.y4m"), str(tmp_path / "clip.gsvc")
    _write_clip(clip, frames_to_u8([cube._image(t) for t in range(T)], fmt).cpu(), H, W, fmt)
    del cube
    log = gsvc_encode.main([clip, "-o", coded, "--steps", "40", "--anchors", "2000", "--slab-frames", "8", "--densify-grad-threshold", "2e-5",
                            "--init", "detail", "--init-cell", "4"])
    assert log["init"] == "detail" and log["init_cell"] == 4 and log["init_mix"] == 0.25 and 0 < log["anchors_initial"] <= 2000
    assert log["total_bytes"] == os.path.getsize(coded)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gsvc_decode.py"), coded, "-o", out, "--strict"], cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-2500:])
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["frames_verified"] == T and line["frames_mismatched"] == 0
