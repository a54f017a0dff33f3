"""GPU tests of the deep (10 / 12 / 16-bit) frame formats: the k_frames_*16 kernels of csrc/frames_out.hip and csrc/frames_in.hip
against the float64 reference of tests/_frames_hbd_ref.py and, exactly, against the 8-bit kernels; what is built on them
(``frames_to_u8`` / ``frames_from_u8`` with ``fmt.depth``, ``delivered_images``, ``render_frames_u8``, ``Y4MWriter``, ``open_video``,
``VideoFileCube``, ``report.evaluate(delivered=...)``).

The conditions (their derivation: tests/_frames_hbd_ref.py):
  * output: every code b against the float64 value v before rounding — nearest |b - v| <= 0.5 + 2^(d - 19), trunc within one level
    (v - 1 - 2^(d - 19) < b <= v + 2^(d - 19)); the upper 16 - d bits of every word zero; guard bytes untouched;
  * limited range, trunc: code_d >> (d - 8) IS the 8-bit kernel's code (the value before rounding is the 8-bit value times 2^(d - 8));
  * input: every float within 2^-20 of the float64 value and inside [0, 1]; a limited-range 8-bit frame and the deep frame of its codes
    times 2^(d - 8) give the same bits;
  * wide path and edge path: the same bits;
  * delivered_images: max |x' - x| <= 2.8556 * 0.5 / (2^d - 1) + 2^-19 for 4:4:4 full range nearest BT.709.
GSVC_PRINT_ERRORS=1 prints each measured figure before it is asserted."""
import functools
import os

import numpy as np
import pytest
import torch

from gsvc_amd import frames_in as fi
from gsvc_amd import frames_out as fo
from gsvc_amd.frames_out import FrameFormat
from tests import _frames_hbd_ref as ref

pytestmark = pytest.mark.gpu
COMBOS = [(m, r) for m in ("bt709", "bt601") for r in ("limited", "full")]
LAYOUTS = ("yuv444p", "yuv420p")
DEPTHS = (10, 12, 16)
GUARD = 0x5A


def _say(what, value):
    if os.environ.get("GSVC_PRINT_ERRORS"):
        print(f"{what}: {value}")


def _words(buf):
    """uint8 tensor (any device) [..., 2 k] -> int64 numpy codes [..., k] (little-endian 16-bit words)."""
    a = np.ascontiguousarray(buf.cpu().numpy())
    return a.view("<u2").astype(np.int64)


def _device_frames(codes, depth):
    """int codes [n, frame_codes] -> uint8 CUDA tensor [n, frame_bytes]."""
    codes = np.asarray(codes)
    return torch.from_numpy(np.stack([ref.to_bytes(c, depth) for c in codes.reshape(-1, codes.shape[-1])])).cuda()


# ---- 1. output against float64 -----------------------------------------------------------------------------------------------------
#        (n, H, W): 2x2, 2x34 and 18x50 take the edge path, 6x48 and 32x64 the wide one; 17 images are two launches
CASES = [(3, 2, 2), (3, 2, 34), (3, 6, 48), (3, 18, 50), (1, 32, 64), (16, 32, 64), (17, 32, 64)]


@functools.lru_cache(maxsize=None)
def _images(n, H, W, depth):
    img = ref.make_images(n, H, W, depth, seed=H + W)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _on_device(n, H, W, depth):
    return torch.from_numpy(np.array(_images(n, H, W, depth))).cuda()


@functools.lru_cache(maxsize=None)
def _values(n, H, W, depth, layout, matrix, rng):
    v = np.stack([ref.values(img, layout, matrix, rng, depth) for img in _images(n, H, W, depth)])
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("rounding", ["trunc", "nearest"])
@pytest.mark.parametrize("matrix,rng", COMBOS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_output_against_float64(layout, matrix, rng, rounding, depth):
    fmt = FrameFormat(layout, matrix, rng, rounding, depth)
    top = 2 ** depth - 1
    for n, H, W in CASES:
        nb = fo.frame_bytes(H, W, fmt)
        pad = 16          # (keeps the stride a multiple of 16 where the frame is: the wide sizes stay on the wide path)
        store = torch.full((n, nb + pad), GUARD, dtype=torch.uint8, device="cuda")
        got = fo.frames_to_u8(_on_device(n, H, W, depth), fmt, out=store)
        assert got.data_ptr() == store.data_ptr() and tuple(got.shape) == (n, nb)
        back = store.cpu()
        assert bool((back[:, nb:] == GUARD).all()), (n, H, W)          # guard bytes behind each frame and between strided frames
        codes = _words(back[:, :nb])
        assert codes.shape == (n, ref.frame_codes(H, W, layout))
        assert int(codes.max()) <= top, (n, H, W, int(codes.max()))          # the upper 16 - d bits are zero in every word
        bad, worst = ref.check_codes(codes, _values(n, H, W, depth, layout, matrix, rng).reshape(-1), rounding, depth)
        _say(f"{fmt.name} {matrix} {rng} {rounding} n={n} {H}x{W} worst excess over the bound", f"{worst:.3e}")
        assert bad == 0, (n, H, W, bad, worst)
        # a plain call (a buffer of its own, stride = frame_bytes): the same bytes
        assert torch.equal(fo.frames_to_u8(_on_device(n, H, W, depth), fmt).cpu(), back[:, :nb])


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_output_of_nan_and_infinities(layout, depth):
    H, W = 4, 8
    img = np.full((3, 3, H, W), 0.25, np.float32)
    img[0, :, :2, :2], img[1, :, :2, :2], img[2, :, :2, :2] = np.nan, -np.inf, np.inf          # one whole 2x2 block each, all channels
    dev = torch.from_numpy(img).cuda()
    top = 2 ** depth - 1
    for rounding in ("trunc", "nearest"):
        # (white is exact under trunc as well: fma(kr, 1, fma(kg, 1, kb)) with the float32 weights of BT.709 and of BT.601 is 1.0)
        full = FrameFormat(layout, "bt709", "full", rounding, depth)
        y = [fo.planes(fr, H, W, full)[0].cpu().numpy().astype(np.int64) for fr in fo.frames_to_u8(dev, full)]
        assert (y[0][:2, :2] == 0).all() and (y[1][:2, :2] == 0).all()          # NaN, -inf: luma code 0
        assert (y[2][:2, :2] == top).all()          # +inf: the top code
        lim = FrameFormat(layout, "bt709", "limited", rounding, depth)
        frames = fo.frames_to_u8(dev, lim)
        yl = [fo.planes(fr, H, W, lim)[0].cpu().numpy().astype(np.int64) for fr in frames]
        up = 2 ** (depth - 8)
        assert (yl[0][:2, :2] == 16 * up).all() and (yl[1][:2, :2] == 16 * up).all()
        assert (yl[2][:2, :2] == 235 * up).all()
        for k in range(3):          # and every code, chroma included, is what the reference says a clamped input gives
            bad, worst = ref.check_codes(_words(frames[k]), ref.values(img[k], layout, "bt709", "limited", depth), rounding, depth)
            assert bad == 0, (k, bad, worst)


# ---- 2. output tied to the 8-bit kernels (exact) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_limited_trunc_codes_shift_down_to_the_8_bit_codes(layout, matrix, depth):
    for n, H, W in ((3, 6, 48), (3, 18, 50), (3, 2, 2), (16, 32, 64)):
        dev = _on_device(n, H, W, depth)
        deep = _words(fo.frames_to_u8(dev, FrameFormat(layout, matrix, "limited", "trunc", depth)))
        eight = fo.frames_to_u8(dev, FrameFormat(layout, matrix, "limited", "trunc")).cpu().numpy().astype(np.int64)
        assert deep.shape == eight.shape
        differing = int(((deep >> (depth - 8)) != eight).sum())
        _say(f"{layout} {matrix} d={depth} n={n} {H}x{W} codes that do not shift down to the 8-bit code", differing)
        assert differing == 0          # no element is left out


# ---- 3. input against float64 ------------------------------------------------------------------------------------------------------
def _axis(depth):
    """The chroma lattice of one axis: 0, 2^(d-1) - 1, 2^(d-1), 2^(d-1) + 1, 2^d - 1 and 11 evenly spaced codes."""
    top, half = 2 ** depth - 1, 2 ** (depth - 1)
    return np.unique(np.concatenate([[0, half - 1, half, half + 1, top], np.round(np.linspace(0, top, 11)).astype(np.int64)]))


def _luma_codes(depth):
    if depth < 16:
        return np.arange(2 ** depth, dtype=np.int64)
    around = np.concatenate([c + np.arange(-32, 33) for c in (0, 16 * 256, 235 * 256, 65535)])
    luma = np.unique(np.concatenate([np.arange(0, 65536, 16), around[(around >= 0) & (around <= 65535)]]))
    return np.concatenate([luma, np.full(-len(luma) % 16, luma[-1])])          # W a multiple of 16


@functools.lru_cache(maxsize=None)
def _lattice(depth):
    """(codes [3, H, W] as a yuv444p frame, H, W): row r holds every luma code against the chroma pair r of the lattice."""
    luma, ax = _luma_codes(depth), _axis(depth)
    assert len(ax) >= 11 and len(luma) % 16 == 0
    cb, cr = (v.reshape(-1) for v in np.meshgrid(ax, ax, indexing="ij"))
    H, W = len(cb), len(luma)
    assert H * W < 2 ** 23
    frame = np.stack([np.broadcast_to(luma[None, :], (H, W)), np.broadcast_to(cb[:, None], (H, W)), np.broadcast_to(cr[:, None], (H, W))])
    frame.setflags(write=False)
    return frame, H, W


@functools.lru_cache(maxsize=None)
def _lattice_on_device(depth):
    frame, H, W = _lattice(depth)
    return _device_frames(frame.reshape(1, -1), depth)


def _check_floats(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    worst = float(np.abs(got.astype(np.float64) - want).max())
    _say(f"{what} max |kernel - float64|", f"{worst:.3e} ({worst / 2.0 ** -24:.2f} x 2^-24)")
    assert worst <= ref.TOL_IN, (what, worst)
    assert got.min() >= 0.0 and got.max() <= 1.0, (what, float(got.min()), float(got.max()))


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("matrix,rng", COMBOS)
def test_input_444_lattice_against_float64(matrix, rng, depth):
    frame, H, W = _lattice(depth)
    out = fi.frames_from_u8(_lattice_on_device(depth), H, W, FrameFormat("yuv444p", matrix, rng, depth=depth))
    assert tuple(out.shape) == (1, 3, H, W)
    _check_floats(out[0].cpu().numpy(), ref.rgb_of_codes(frame[0], frame[1], frame[2], matrix, rng, depth), f"444 lattice d={depth} {matrix} {rng}")


SIZES_420 = [(2, 2), (4, 6), (16, 32), (18, 50)]


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("chroma", ["bilinear", "nearest"])
def test_input_420_random_codes_against_float64(chroma, depth):
    for H, W in SIZES_420:
        codes = np.stack([ref.random_codes(H, W, "yuv420p", depth, 10 * k + H) for k in range(3)])
        dev = _device_frames(codes, depth)
        for matrix, rng in COMBOS:
            out = fi.frames_from_u8(dev, H, W, FrameFormat("yuv420p", matrix, rng, depth=depth), chroma=chroma).cpu().numpy()
            for k in range(3):
                _check_floats(out[k], ref.image(codes[k], H, W, "yuv420p", matrix, rng, chroma, depth), f"420 {chroma} d={depth} {matrix} {rng} {H}x{W} [{k}]")


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("chroma", ["bilinear", "nearest"])
@pytest.mark.parametrize("size", [(16, 32), (18, 50)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_input_420_single_chroma_samples_bit_for_bit(size, chroma, depth):
    """Full range, luma 0; one chroma plane neutral (2^(d-1): C = 0), the other 0 except ONE sample of 2^d - 1, at each corner and in
    the interior.  The interpolated codes are exact in float32, C = (c - 2^(d-1)) / (2^d - 1) is one correctly rounded division and,
    with Y = 0 and the other C = 0, every channel is ONE correctly rounded product — so numpy float32 states the kernel's bits, and the
    clamped-index weights show in them exactly."""
    H, W = size
    h, w = H // 2, W // 2
    top, half = 2 ** depth - 1, 2 ** (depth - 1)
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2), (1, w - 2)]
    frames, ups = [], []
    for plane in (0, 1):
        for i, j in spots:
            c = np.zeros((h, w), np.int64)
            c[i, j] = top
            other = np.full((h, w), half, np.int64)
            u, v = (c, other) if plane == 0 else (other, c)
            frames.append(np.concatenate([np.zeros(H * W, np.int64), u.reshape(-1), v.reshape(-1)]))
            ups.append((ref.upsample_codes(u, chroma), ref.upsample_codes(v, chroma)))
    for matrix in ("bt709", "bt601"):
        out = fi.frames_from_u8(_device_frames(np.stack(frames), depth), H, W, FrameFormat("yuv420p", matrix, "full", depth=depth), chroma=chroma).cpu().numpy()
        Kr, Kb = ref.MATRIX[matrix]
        Kg = 1.0 - Kr - Kb
        f = np.float32
        r_cr, b_cb = f(2.0 * (1.0 - Kr)), f(2.0 * (1.0 - Kb))
        g_cr, g_cb = f(2.0 * Kr * (1.0 - Kr) / Kg), f(2.0 * Kb * (1.0 - Kb) / Kg)
        for k, (uu, vv) in enumerate(ups):
            assert np.array_equal(uu.astype(f).astype(np.float64), uu)          # the interpolated codes are float32 numbers
            Cb, Cr = (uu.astype(f) - f(half)) / f(top), (vv.astype(f) - f(half)) / f(top)
            assert Cb.dtype == np.float32
            want = np.stack([r_cr * Cr, -g_cb * Cb if k < len(spots) else -g_cr * Cr, b_cb * Cb])
            want = np.clip(want, f(0), f(1)).astype(f)
            assert np.array_equal(out[k], want), (matrix, k, int((out[k] != want).sum()))


# ---- 4. input tied to the 8-bit kernels (exact) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
@pytest.mark.parametrize("layout,chroma", [("yuv444p", "bilinear"), ("yuv420p", "bilinear"), ("yuv420p", "nearest")])
def test_limited_8_bit_frame_and_its_scaled_deep_frame_give_the_same_bits(layout, chroma, matrix, depth):
    for H, W in ((16, 32), (18, 50)):
        eight = np.stack([ref.random_codes(H, W, layout, 8, 20 * k + W) for k in range(3)])
        a = fi.frames_from_u8(_device_frames(eight, 8), H, W, FrameFormat(layout, matrix, "limited"), chroma=chroma)
        b = fi.frames_from_u8(_device_frames(eight * 2 ** (depth - 8), depth), H, W, FrameFormat(layout, matrix, "limited", depth=depth), chroma=chroma)
        assert float(a.std()) > 0.1 and torch.equal(a, b), (H, W)


# ---- 5. wide path and edge path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_wide_and_edge_paths_give_the_same_bits(layout, depth):
    n, H, W = 3, 6, 48
    for matrix, rng in COMBOS:
        fmt = FrameFormat(layout, matrix, rng, depth=depth)
        nb = fo.frame_bytes(H, W, fmt)
        assert nb % 16 == 0
        codes = np.stack([ref.random_codes(H, W, layout, depth, 30 * k + depth) for k in range(n)])
        aligned = _device_frames(codes, depth)
        room = torch.empty(n * nb + 16, dtype=torch.uint8, device="cuda")
        shifted = room[2:2 + n * nb].view(n, nb)          # a view shifted by 2 bytes: the edge path
        shifted.copy_(aligned)
        assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 2
        for chroma in (("bilinear", "nearest") if layout == "yuv420p" else ("bilinear",)):
            wide = fi.frames_from_u8(aligned, H, W, fmt, chroma=chroma)
            edge = fi.frames_from_u8(shifted, H, W, fmt, chroma=chroma)
            assert torch.equal(wide, edge), (matrix, rng, chroma)
        # output: into an aligned buffer and into a shifted one, identical bytes; the bytes around the shifted frames stay
        images = _on_device(n, H, W, depth)
        for rounding in ("trunc", "nearest"):
            ofmt = FrameFormat(layout, matrix, rng, rounding, depth)
            plain = fo.frames_to_u8(images, ofmt)
            room = torch.full((n * nb + 16,), GUARD, dtype=torch.uint8, device="cuda")
            view = room[2:2 + n * nb].view(n, nb)
            assert plain.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 2
            fo.frames_to_u8(images, ofmt, out=view)
            assert torch.equal(view, plain), (matrix, rng, rounding)
            assert bool((room[:2] == GUARD).all()) and bool((room[2 + n * nb:] == GUARD).all())


def test_odd_bases_and_strides_are_refused():
    from gsvc_amd import _lib
    fmt = FrameFormat("yuv444p", depth=10)
    H, W = 4, 8
    nb = fo.frame_bytes(H, W, fmt)
    room = torch.zeros(3 * nb + 8, dtype=torch.uint8, device="cuda")
    images = torch.zeros(2, 3, H, W, device="cuda")
    with pytest.raises(_lib.GsvcError, match="2-byte aligned"):
        fi.frames_from_u8(room[1:1 + nb], H, W, fmt)
    with pytest.raises(_lib.GsvcError, match="2-byte aligned"):
        fo.frames_to_u8(images[:1], fmt, out=room[1:1 + nb].view(1, nb))
    with pytest.raises(_lib.GsvcError, match="multiple of 2"):
        fi.frames_from_u8(room[:2 * (nb + 1)].view(2, nb + 1)[:, :nb], H, W, fmt)
    with pytest.raises(_lib.GsvcError, match="multiple of 2"):
        fo.frames_to_u8(images, fmt, out=room[:2 * (nb + 1)].view(2, nb + 1))
    with pytest.raises(ValueError, match="even"):
        fi.frames_from_u8(room[:36], 3, 4, FrameFormat("yuv420p", depth=10))


# ---- 6. delivered_images ------------------------------------------------------------------------------------------------------------
def test_delivered_images_round_trip_bound():
    H, W = 32, 64
    x = torch.from_numpy(np.random.default_rng(17).uniform(0.0, 1.0, (4, 3, H, W)).astype(np.float32)).cuda()
    worst = {}
    for depth in (8, 10, 12, 16):
        back = fo.delivered_images(x, FrameFormat("yuv444p", "bt709", "full", "nearest", depth))
        assert back.dtype == torch.float32 and tuple(back.shape) == (4, 3, H, W)
        worst[depth] = float((back.double() - x.double()).abs().max())
        bound = 2.8556 * 0.5 / (2 ** depth - 1) + 2.0 ** -19
        _say(f"delivered yuv444p full nearest bt709 d={depth} max |x' - x|", f"{worst[depth]:.4e} (bound {bound:.4e})")
        assert worst[depth] <= bound, (depth, worst[depth], bound)
    assert worst[10] < worst[8]
    # a list of images and 4:2:0 go through as well
    got = fo.delivered_images(list(x.unbind(0)), FrameFormat("yuv420p", depth=10), chroma="nearest")
    assert tuple(got.shape) == (4, 3, H, W) and float((got - x).abs().mean()) < 0.2


def test_delivered_rgb24_is_what_evaluate_eight_bit_forms():
    H, W = 34, 50
    x = torch.from_numpy(np.random.default_rng(18).uniform(-0.1, 1.1, (3, 3, H, W)).astype(np.float32)).cuda()
    images = [torch.clamp(img, 0.0, 1.0) for img in x]
    today = [fo.rgb24_to_image(u8, H, W) for u8 in fo.frames_to_u8(images, FrameFormat("rgb24", rounding="trunc"))]
    got = fo.delivered_images(images, FrameFormat("rgb24"))
    assert tuple(got.shape) == (3, 3, H, W) and all(torch.equal(a, b) for a, b in zip(got.unbind(0), today))


# ---- 7. files and the fit -----------------------------------------------------------------------------------------------------------
def test_y4m_writer_and_open_video_carry_10_bit_frames(tmp_path):
    H, W, T = 18, 50, 5
    fmt = FrameFormat("yuv420p", depth=10)
    u8 = fo.frames_to_u8(_on_device(16, 32, 64, 10)[:T, :, :H, :W], fmt)
    with fo.Y4MWriter(tmp_path / "v.y4m", W, H, (30, 1), fmt) as sink:
        for fr in u8.cpu():
            sink.write(fr)
    assert (tmp_path / "v.y4m").read_bytes().split(b"\n", 1)[0].split(b" ")[6] == b"C420p10"
    hdr, back = fi.open_video(tmp_path / "v.y4m")
    assert hdr["fmt"] == fmt and (hdr["W"], hdr["H"], hdr["frames"], hdr["depth"]) == (W, H, T, 10)
    assert np.array_equal(back, u8.cpu().numpy())
    for resident in ("float", "u8"):
        cube = fi.VideoFileCube(tmp_path / "v.y4m", resident=resident)
        assert cube.fmt == fmt
        want = fi.frames_from_u8(u8, H, W, fmt)
        for i in range(T):
            assert torch.equal(cube[i].image, want[i].permute(0, 2, 1))


def test_fit_from_a_10_bit_file_is_the_same_fit_whatever_the_residency(tmp_path, monkeypatch):
    """The residency test of tests/test_frames_in_gpu.py, its sizes, on a 10-bit Y4M file."""
    from gsvc_amd import switches
    from gsvc_amd.train import Trainer
    from tests.test_frames_in_gpu import _small_model, _synthetic_video
    H, W, T = 96, 160, 12
    fmt = FrameFormat("yuv420p", depth=10)
    _synthetic_video(tmp_path / "v.y4m", H, W, T, fmt)
    assert b" C420p10 " in (tmp_path / "v.y4m").read_bytes()[:80]

    def fit(resident):
        cube = fi.VideoFileCube(tmp_path / "v.y4m", resident=resident)
        assert cube.fmt == fmt and cube.header["frame_bytes"] == H * W * 3
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
        tr.close()
        return [float(x) for x in losses], state

    monkeypatch.setenv("GSVC_DETERMINISTIC", "1")
    switches.reload()
    try:
        l_float, s_float = fit("float")
        l_u8, s_u8 = fit("u8")
    finally:
        monkeypatch.delenv("GSVC_DETERMINISTIC", raising=False)
        switches.reload()
    assert all(np.isfinite(l_float)) and l_float == l_u8
    differing = [n for n in s_float if not torch.equal(s_float[n], s_u8[n])]
    assert not differing, differing


def test_render_frames_u8_delivers_10_bit_frames_and_evaluate_takes_a_delivered_format():
    from gsvc_amd.ortho_gaussian_renderer import render_frames
    from gsvc_amd.report import evaluate
    from tests.test_frames_out_gpu import _fitted
    H, W = 96, 160
    pc, cube, pipe = _fitted(H, W)
    bg = torch.zeros(3)
    fmt = FrameFormat("yuv420p", depth=10)
    nb = fo.frame_bytes(H, W, fmt)
    assert nb == 2 * fo.frame_bytes(H, W, FrameFormat("yuv420p"))
    for batch, count in ((3, 7), (8, 5)):
        frames = [cube.get_dummy_frame(i) for i in range(1, 1 + count)]
        want = fo.frames_to_u8(list(render_frames(frames, pc, pipe, bg, batch=batch)), fmt)
        assert float(_words(want).std()) > 4.0          # not flat
        on_dev = list(fo.render_frames_u8(frames, pc, pipe, bg, fmt=fmt, batch=batch, to_host=False))
        assert len(on_dev) == count and all(f.is_cuda and tuple(f.shape) == (nb,) for f in on_dev)
        assert torch.equal(torch.stack(on_dev), want)
        on_host = [f.clone() for f in fo.render_frames_u8(frames, pc, pipe, bg, fmt=fmt, batch=batch, to_host=True)]
        assert len(on_host) == count and all(not f.is_cuda and f.dtype == torch.uint8 for f in on_host)
        assert torch.equal(torch.stack(on_host), want.cpu()), (batch, count)
    ids = [2, 3, 4]
    plain = evaluate(pc, cube, pipe, bg, frame_ids=ids)
    eight = evaluate(pc, cube, pipe, bg, frame_ids=ids, eight_bit=True)
    as_rgb = evaluate(pc, cube, pipe, bg, frame_ids=ids, delivered=FrameFormat("rgb24"))
    assert as_rgb["delivered"] == "rgb24" and "eight_bit" not in as_rgb and "delivered" not in eight and "delivered" not in plain
    assert (as_rgb["psnr"], as_rgb["ssim"], as_rgb["l1"]) == (eight["psnr"], eight["ssim"], eight["l1"])
    deep = evaluate(pc, cube, pipe, bg, frame_ids=ids, delivered=FrameFormat("yuv444p", range="full", depth=10))
    assert deep["delivered"] == "yuv444p10le" and np.isfinite(deep["psnr"]) and abs(deep["psnr"] - plain["psnr"]) < 0.5
    with pytest.raises(ValueError, match="give one"):
        evaluate(pc, cube, pipe, bg, frame_ids=ids, eight_bit=True, delivered=fmt)
