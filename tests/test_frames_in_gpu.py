"""GPU tests of the encoder's 8-bit input stage: the kernels of csrc/frames_in.hip against the float64 reference of
tests/_frames_in_ref.py, and what is built on them (gsvc_amd/frames_in.py: ``frames_from_u8``, ``VideoFileCube``; tools/fit_synthetic.py
--video).

The conditions:
  * every output element within TOL = 2^-20 of the float64 value and inside [0, 1] (the derivation: tests/_frames_in_ref.py; the
    honest float32 evaluation is within 2.2e-7 = 2^-22.1 over all 2^24 code triples);
  * rgb24 bit-equal to ``bytes.float().div(255)``;
  * whichever path a frame takes (wide: W a multiple of 16 and 16-byte-aligned bases and stride; edge: anything else), the same bits;
  * only the images are written: guard floats around them come back untouched;
  * bytes -> floats -> bytes gives the bytes back (rgb24; 4:4:4 for images inside the gamut);
  * a fit reads the same pictures from a file whether they are resident as float or as bytes: same parameters, bit for bit.
GSVC_PRINT_ERRORS=1 prints each measured figure before it is asserted."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from gsvc_amd import frames_in as fi
from gsvc_amd import frames_out as fo
from gsvc_amd.frames_out import FrameFormat
from tests import _frames_in_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = ref.TOL
COMBOS = [(m, r) for m in ("bt709", "bt601") for r in ("limited", "full")]
LAYOUTS = ("rgb24", "yuv444p", "yuv420p")


def _say(what, value):
    if os.environ.get("GSVC_PRINT_ERRORS"):
        print(f"{what}: {value}")


def _check(got, want, what):
    """got: float32 numpy [3, H, W] of the kernel; want: float64 of the reference."""
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    worst = float(np.abs(got.astype(np.float64) - want).max())
    _say(f"{what} max |kernel - float64|", f"{worst:.3e} ({worst / 2.0 ** -24:.2f} x 2^-24)")
    assert worst <= TOL, (what, worst)
    assert got.min() >= 0.0 and got.max() <= 1.0, (what, float(got.min()), float(got.max()))


@functools.lru_cache(maxsize=None)
def _frame(H, W, layout, seed):
    fr = ref.random_frame(H, W, layout, seed)
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def _want(H, W, layout, seed, matrix="bt709", rng="limited", chroma="bilinear"):
    v = ref.values(_frame(H, W, layout, seed), H, W, layout, matrix, rng, chroma)
    v.setflags(write=False)
    return v


# ---- 1. every code triple ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _all_triples_on_device():
    frame = torch.from_numpy(ref.all_triples_frame())
    aligned = frame.cuda()
    shifted = torch.empty(frame.numel() + 1, dtype=torch.uint8, device="cuda")[1:]          # a base that is 1-byte aligned: the edge path
    shifted.copy_(frame)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 1
    return aligned, shifted


@pytest.mark.parametrize("matrix,rng", COMBOS)
def test_every_code_triple_444(matrix, rng):
    S = 4096
    aligned, shifted = _all_triples_on_device()
    fmt = FrameFormat("yuv444p", matrix, rng)
    wide = fi.frames_from_u8(aligned, S, S, fmt)
    edge = fi.frames_from_u8(shifted, S, S, fmt)
    assert tuple(wide.shape) == (1, 3, S, S) and wide.dtype == torch.float32
    assert torch.equal(wide, edge)          # which path a frame takes does not change a bit
    got = wide[0].cpu().numpy().reshape(3, -1)
    assert got.min() >= 0.0 and got.max() <= 1.0
    worst, step = 0.0, 1 << 20
    for at in range(0, S * S, step):          # in pieces: the float64 intermediates of 2^24 triples at once are gigabytes
        p = np.arange(at, at + step, dtype=np.int64)
        want = ref.rgb_of_codes(p & 255, (p >> 8) & 255, p >> 16, matrix, rng)
        worst = max(worst, float(np.abs(got[:, at:at + step].astype(np.float64) - want).max()))
    _say(f"all triples {matrix} {rng} max |kernel - float64|", f"{worst:.3e} ({worst / 2.0 ** -24:.2f} x 2^-24)")
    assert worst <= TOL, worst


# ---- 2. rgb24 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (3, 5), (16, 16), (34, 50), (270, 480)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rgb24_is_bit_equal_to_div_255(size, tmp_path):
    """Enough frames that every byte value stands at every position modulo 16 of a frame (at every position, where a frame has fewer
    than 16 bytes): value(frame k, byte i) = (i / 16 + 17 (i mod 16) + k B) mod 256 with B the frame's whole 16-byte blocks."""
    H, W = size
    L = 3 * H * W
    B = max(L // 16, 1)
    n = -(-256 // B)
    i, k = np.arange(L, dtype=np.int64)[None, :], np.arange(n, dtype=np.int64)[:, None]
    frames = (((i >> 4) + 17 * (i & 15) + k * B) & 255).astype(np.uint8)
    for p in range(min(L, 16)):
        assert len(np.unique(frames[:, p::16])) == 256
    fmt = FrameFormat("rgb24")
    dev = torch.from_numpy(frames).cuda()
    out = fi.frames_from_u8(dev, H, W, fmt)
    want = torch.from_numpy(frames).view(n, H, W, 3).float().div(255).permute(0, 3, 1, 2).contiguous()
    assert tuple(out.shape) == (n, 3, H, W) and torch.equal(out.cpu(), want)
    # a frame at a 1-byte-aligned base (the edge path at the wide sizes): the same bits
    shifted = torch.empty(L + 1, dtype=torch.uint8, device="cuda")[1:]
    shifted.copy_(dev[0])
    assert torch.equal(fi.frames_from_u8(shifted, H, W, fmt)[0], out[0])
    # and what the PNG path of the project gives for the same bytes
    from PIL import Image
    from gsvc_amd.io import load_image
    Image.fromarray(frames[0].reshape(H, W, 3), "RGB").save(tmp_path / "f.png")
    assert torch.equal(load_image(tmp_path / "f.png"), out[0].cpu())


# ---- 3. 4:2:0 -----------------------------------------------------------------------------------------------------------------------
SIZES_420 = [(2, 2), (2, 8), (4, 6), (6, 10), (16, 16), (18, 34), (32, 64), (34, 50), (270, 480)]


@pytest.mark.parametrize("matrix,rng", COMBOS)
@pytest.mark.parametrize("chroma", ["bilinear", "nearest"])
@pytest.mark.parametrize("size", SIZES_420, ids=lambda s: f"{s[0]}x{s[1]}")
def test_420_against_float64(size, chroma, matrix, rng):
    H, W = size
    frames = [np.array(_frame(H, W, "yuv420p", H + W)), ref.checkerboard_frame(H, W, H + W)]
    fmt = FrameFormat("yuv420p", matrix, rng)
    out = fi.frames_from_u8(torch.from_numpy(np.stack(frames)).cuda(), H, W, fmt, chroma=chroma)
    assert torch.equal(out, fi.frames_from_u8(torch.from_numpy(np.stack(frames)).cuda(), H, W, fmt, chroma=chroma))
    got = out.cpu().numpy()
    for k, (kind, fr) in enumerate(zip(("noise", "checkerboard"), frames)):
        what = f"420 {chroma} {matrix} {rng} {H}x{W} {kind}"
        _check(got[k], ref.values(fr, H, W, "yuv420p", matrix, rng, chroma), what)
        if chroma == "bilinear":
            # the second, independent statement of the upsampling: torch's bilinear interpolation of the code planes on the CPU
            y, u, v = ref.split(fr, H, W, "yuv420p")
            up = [torch.nn.functional.interpolate(torch.from_numpy(c.astype(np.float64))[None, None], scale_factor=2, mode="bilinear",
                                                  align_corners=False)[0, 0].numpy() for c in (u, v)]
            _check(got[k], ref.rgb_of_codes(y, up[0], up[1], matrix, rng), what + " (F.interpolate)")
    # a frame at a 1-byte-aligned base takes the edge path: the same bits (at the wide sizes this compares the two paths)
    L = ref.frame_bytes(H, W, "yuv420p")
    shifted = torch.empty(L + 1, dtype=torch.uint8, device="cuda")[1:]
    shifted.copy_(torch.from_numpy(frames[1]))
    assert torch.equal(fi.frames_from_u8(shifted, H, W, fmt, chroma=chroma)[0], out[1])


def test_420_refuses_odd_sizes():
    with pytest.raises(ValueError, match="even"):
        fi.frames_from_u8(torch.zeros(1, 64, dtype=torch.uint8, device="cuda"), 3, 4, FrameFormat("yuv420p"))


# ---- 4. batches, strides, guards ----------------------------------------------------------------------------------------------------
GUARD = -7.25
#          (H, W), bytes between frames, input base offset, floats before the first image, floats between images
SETUPS = [((32, 64), 64, 0, 8, 8),          # everything 16-byte aligned: the wide path, around guards
          ((32, 64), 13, 0, 8, 8),          # a stride that is no multiple of 16
          ((32, 64), 64, 1, 8, 8),          # frames at 1-byte-aligned bases
          ((32, 64), 64, 0, 5, 7),          # images at bases that are 4-byte but not 16-byte aligned
          ((34, 50), 13, 1, 5, 7)]          # no multiple of the lane's pixels, nothing aligned


@pytest.mark.parametrize("n", [1, 3, 8, 16, 17, 33])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_batch_sizes_strides_and_guard_floats(layout, n):
    fmt = FrameFormat(layout)
    for (H, W), pad, off, lead, gap in SETUPS:
        L, px = ref.frame_bytes(H, W, layout), 3 * H * W
        host = np.full((n, L + pad), 0x5A, np.uint8)
        for k in range(n):
            host[k, :L] = _frame(H, W, layout, k)
        buf = torch.empty(off + n * (L + pad), dtype=torch.uint8, device="cuda")
        src = buf[off:].view(n, L + pad)
        src.copy_(torch.from_numpy(host))
        store = torch.full((lead + n * (px + gap) + 40,), GUARD, dtype=torch.float32, device="cuda")
        out = store[lead:lead + n * (px + gap)].view(n, px + gap)[:, :px].view(n, 3, H, W)
        assert src.data_ptr() % 16 == off and out.data_ptr() % 16 == (4 * lead) % 16
        ret = fi.frames_from_u8(src, H, W, fmt, out=out)
        assert ret.data_ptr() == out.data_ptr() and tuple(ret.shape) == (n, 3, H, W)
        back = store.cpu().numpy()
        assert (back[:lead] == GUARD).all() and (back[lead + n * (px + gap):] == GUARD).all()
        rows = back[lead:lead + n * (px + gap)].reshape(n, px + gap)
        assert (rows[:, px:] == GUARD).all()
        plain = fi.frames_from_u8(torch.from_numpy(host[:, :L].copy()).cuda(), H, W, fmt).cpu().numpy()
        assert np.array_equal(rows[:, :px].reshape(n, 3, H, W), plain)          # the same floats whichever path, stride and base
        for k in range(n):
            _check(plain[k], _want(H, W, layout, k), f"{layout} n={n} {H}x{W} pad {pad} off {off} [{k}]")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_launch_on_another_stream_and_flat_frame(layout):
    H, W = 32, 64
    fmt = FrameFormat(layout)
    src = torch.from_numpy(np.stack([_frame(H, W, layout, k) for k in range(3)])).cuda()
    plain = fi.frames_from_u8(src, H, W, fmt)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = fi.frames_from_u8(src, H, W, fmt)
    side.synchronize()
    assert torch.equal(plain, other)
    flat = fi.frames_from_u8(src[1], H, W, fmt)          # one flat frame
    assert tuple(flat.shape) == (1, 3, H, W) and torch.equal(flat[0], plain[1])
    with pytest.raises(ValueError):
        fi.frames_from_u8(src.int(), H, W, fmt)
    with pytest.raises(ValueError):
        fi.frames_from_u8(src[:, :-1], H, W, fmt)
    with pytest.raises(ValueError):
        fi.frames_from_u8(src, H, W, fmt, out=torch.empty(3, 3, W, H, device="cuda"))
    with pytest.raises(ValueError):
        fi.frames_from_u8(src, H, W, fmt, out=torch.empty(3, 3, H, W, device="cuda", dtype=torch.float64))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_1080p_batch_of_eight(layout):
    H, W = 1080, 1920
    frames = np.stack([ref.random_frame(H, W, layout, 40 + k) for k in range(8)])
    out = fi.frames_from_u8(torch.from_numpy(frames).cuda(), H, W, FrameFormat(layout)).cpu().numpy()
    for k in range(8):
        _check(out[k], ref.values(frames[k], H, W, layout), f"{layout} 1080p [{k}]")


# ---- 5. round trips with the decoder's direction ------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(34, 50), (32, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_round_trip_rgb24(size):
    H, W = size
    b = torch.from_numpy(np.stack([_frame(H, W, "rgb24", 60 + k) for k in range(3)])).cuda()
    fmt = FrameFormat("rgb24", rounding="nearest")
    again = fo.frames_to_u8(fi.frames_from_u8(b, H, W, fmt), fmt)
    assert int((again != b).sum()) == 0


@pytest.mark.parametrize("matrix,rng", COMBOS)
def test_round_trip_yuv444(matrix, rng):
    """Images uniform in [0.05, 0.95]: the references leave 0 of the 12 288 bytes different and clamp nothing
    (tests/test_frames_in_cpu.py); on [0, 1] the gamut clamp would break the round trip."""
    img = torch.from_numpy(np.random.default_rng(11).uniform(0.05, 0.95, (1, 3, 64, 64)).astype(np.float32)).cuda()
    fmt = FrameFormat("yuv444p", matrix, rng, "nearest")
    b = fo.frames_to_u8(img, fmt)
    assert b.numel() == 12288
    again = fo.frames_to_u8(fi.frames_from_u8(b, 64, 64, fmt), fmt)
    differing = int((again != b).sum())
    _say(f"4:4:4 round trip {matrix} {rng} differing bytes", differing)
    assert differing == 0


# ---- 6. files -----------------------------------------------------------------------------------------------------------------------
def _synthetic_video(path, H, W, T, fmt):
    """The frames of a SyntheticFrameCube written as 8-bit video: (cube, uint8 device frames [T, frame_bytes])."""
    from gsvc_amd.frame import SyntheticFrameCube
    cube = SyntheticFrameCube(H, W, T, device="cuda")
    u8 = fo.frames_to_u8([cube[i].image.permute(0, 2, 1).contiguous() for i in range(T)], fmt)
    sink, _ = fo.open_sink(path, W, H, fmt=fmt)
    with sink:
        for fr in u8.cpu():
            sink.write(fr)
    return cube, u8


@pytest.mark.parametrize("layout", ["yuv420p", "yuv444p"])
def test_video_file_cube_reads_what_the_writer_wrote(layout, tmp_path):
    H, W, T = 96, 160, 6
    fmt = FrameFormat(layout)
    synth, u8 = _synthetic_video(tmp_path / "v.y4m", H, W, T, fmt)
    want = fi.frames_from_u8(u8, H, W, fmt)
    as_float = fi.VideoFileCube(tmp_path / "v.y4m", resident="float")
    as_u8 = fi.VideoFileCube(tmp_path / "v.y4m", resident="u8")
    (tmp_path / "v.yuv").write_bytes(u8.cpu().numpy().tobytes())
    raw = fi.VideoFileCube(tmp_path / "v.yuv", W=W, H=H, fmt=fmt, resident="u8")
    for cube in (as_float, as_u8, raw):
        assert (len(cube), cube.len_z_frames, cube.frame_num, cube.height, cube.width) == (T, T, T, H, W)
        assert (cube.scale, cube.x_min, cube.y_min, cube.z_min) == (synth.scale, synth.x_min, synth.y_min, synth.z_min)
        assert cube.fmt == fmt
        for i in range(T):
            fr, sf = cube[i], synth[i]
            assert tuple(fr.image.shape) == (3, W, H) and fr.image.is_cuda
            assert torch.equal(fr.image, want[i].permute(0, 2, 1))
            assert (fr.image_id, fr.z, fr.image_width, fr.image_height, fr.scale) == (sf.image_id, sf.z, sf.image_width, sf.image_height, sf.scale)
            assert torch.equal(fr.view_matrix, sf.view_matrix) and torch.equal(fr.view_matrix_s, sf.view_matrix_s)
            # the synthetic picture again, 8 bits away: one code of Y is 1/219 and one of Cr 1.575/224 of R, half of each at the
            # most from rounding; the smooth pictures lose far less than that on average to the subsampled chroma
            assert float((fr.image - sf.image).abs().mean()) < 0.01
        assert cube.get_dummy_frame(2).image is None and cube.get_z_frame(3).image_id == 3
        cube.ready(0)
        with pytest.raises(RuntimeError, match="optical_lambda = 0"):
            cube.get_optical_flow(0)
    assert as_float._u8 is None and as_u8._images is None and tuple(as_u8._u8.shape) == (T, fo.frame_bytes(H, W, fmt))
    (tmp_path / "cut.yuv").write_bytes(u8.cpu().numpy().tobytes()[:-5])
    with pytest.raises(ValueError, match="not a whole number"):
        fi.VideoFileCube(tmp_path / "cut.yuv", W=W, H=H, fmt=fmt)


def test_video_file_cube_rgb_file_and_flow_directory(tmp_path):
    H, W, T = 34, 50, 18          # more than one upload chunk
    frames = np.stack([_frame(H, W, "rgb24", 80 + k) for k in range(T)])
    (tmp_path / "v.rgb").write_bytes(frames.tobytes())
    flows = tmp_path / "flow"
    flows.mkdir()
    field = np.random.default_rng(3).normal(size=(T - 1, 2, H, W)).astype(np.float32)
    for k in range(T - 1):
        np.save(flows / f"{k:04d}.npy", field[k])
    want = torch.from_numpy(frames).view(T, H, W, 3).float().div(255).permute(0, 3, 2, 1)          # [T, 3, W, H]
    for resident in ("float", "u8"):
        cube = fi.VideoFileCube(tmp_path / "v.rgb", optical_flow_dir=flows, W=W, H=H, resident=resident)
        assert cube.fmt.layout == "rgb24" and len(cube) == T
        for i in range(T):
            assert torch.equal(cube[i].image.cpu(), want[i])
        assert torch.equal(cube.get_optical_flow(5).cpu(), torch.from_numpy(field[5])) and cube.get_optical_flow(5).is_cuda


# ---- 7. a fit from a file -----------------------------------------------------------------------------------------------------------
def _small_model(cube, seed):
    from gsvc_amd.arguments import ModelParams, OptimizationParams, PipelineParams
    from gsvc_amd.model import GaussianModel
    mp = ModelParams()
    mp.grid_feature_dim = 2
    opt = OptimizationParams()
    opt.lmbda = 0.004
    mp.threshold = 3.0 / cube.scale
    torch.manual_seed(seed)
    np.random.seed(seed)
    pc = GaussianModel(mp, 16, 5, 0.001, 3, 16, 4, False, n_features_per_level=2, log2_hashmap_size=10, log2_hashmap_size_2D=12,
                       resolutions_list=(18, 24, 33, 44), resolutions_list_2D=(130, 258), device="cuda")
    lim = np.array([cube.x_min, cube.y_min, cube.z_min]) * 1.1
    pc.create_from_points(np.random.default_rng(seed).uniform(lim, -lim, (5000, 3)), spatial_lr_scale=1.0)
    pc.update_anchor_bound(cube.x_min, cube.y_min, cube.z_min)
    return pc, opt, PipelineParams(), mp


def test_fit_from_a_file_is_the_same_fit_whatever_the_residency(tmp_path, monkeypatch):
    """12 steps through the four phases under GSVC_DETERMINISTIC=1, from the same Y4M file kept as float pictures and kept as bytes:
    the pixels are the same, only where they live and when they are converted differs — a picture that a later fetch or the
    allocator overwrote under the step's streams would show as different parameters."""
    from gsvc_amd import switches
    from gsvc_amd.report import evaluate
    from gsvc_amd.train import Trainer
    H, W, T = 96, 160, 12
    _synthetic_video(tmp_path / "v.y4m", H, W, T, FrameFormat("yuv420p"))

    def fit(resident):
        cube = fi.VideoFileCube(tmp_path / "v.y4m", resident=resident)
        pc, opt, pipe, mp = _small_model(cube, seed=11)
        opt.optical_lambda = 0.0
        opt.full_precision_training_total, opt.quantized_training_total = 3, 3
        opt.entropy_constrained_train_total, opt.ste_entropy_constrained_train_total = 3, 3
        opt.start_stat, opt.update_until, opt.pause_densification = 0, 10 ** 9, 0
        pc.training_setup(opt)
        tr = Trainer(pc, cube, opt, pipe, mp, seed=3)
        losses = [tr.step(it).loss.detach() for it in range(1, 13)]
        torch.cuda.synchronize()
        state = {n: p.detach().clone() for n, p in pc.named_parameters()}
        state.update({n: getattr(pc, n).clone() for n in ("opacity_accum", "anchor_demon", "offset_gradient_accum", "offset_denom")})
        with torch.no_grad():
            ev = evaluate(pc, cube, pipe, tr.background, frame_ids=[0, 5, 11])
        tr.close()
        return [float(x) for x in losses], state, ev

    monkeypatch.setenv("GSVC_DETERMINISTIC", "1")
    switches.reload()
    try:
        l_float, s_float, ev_float = fit("float")
        l_u8, s_u8, ev_u8 = fit("u8")
    finally:
        monkeypatch.delenv("GSVC_DETERMINISTIC", raising=False)
        switches.reload()
    assert all(np.isfinite(l_float)) and l_float == l_u8
    differing = [n for n in s_float if not torch.equal(s_float[n], s_u8[n])]
    assert not differing, differing
    assert np.isfinite(ev_float["psnr"]) and ev_float["psnr"] == ev_u8["psnr"]


# ---- 8. the tool ----------------------------------------------------------------------------------------------------------------------
def test_fit_tool_takes_a_video_file(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fit_synthetic
    H, W, T = 272, 480, 24          # (the size of tests/test_fit_tool_gpu.py)
    _synthetic_video(tmp_path / "that.y4m", H, W, T, FrameFormat("yuv420p"))
    out = tmp_path / "rd.json"
    # (returns = exit status 0; the payload identity of an 8-step model is not this test's subject: tests/test_fit_tool_gpu.py holds it)
    fit_synthetic.main(["--video", str(tmp_path / "that.y4m"), "--steps", "8", "--anchors", "8000", "--eval-frames", "4", "--slab-frames", "8",
                        "--video-resident", "u8", "--payload-tol", "1e9", "--json", str(out)])
    log = json.loads(out.read_text())
    assert log["video"]["frames"] == T and (log["video"]["W"], log["video"]["H"]) == (W, H)
    assert (log["config"]["frames"], log["config"]["W"], log["config"]["H"]) == (T, W, H)
    assert log["video"]["optical_lambda"] == 0.0 and log["video"]["layout"] == "yuv420p" and log["video"]["resident"] == "u8"
    assert np.isfinite(log["decoded_8bit_mlp"]["psnr"])
