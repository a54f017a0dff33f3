"""GPU tests of the decoder's 8-bit output stage: the kernel of csrc/frames_out.hip against the float64 reference of
tests/_frames_ref.py, and the loop / sink / evaluation code built on it (gsvc_amd/frames_out.py, report.evaluate(eight_bit=True),
tools/fit_synthetic.py --write-decoded).

The conditions on the bytes (v = the float64 value before rounding, delta = 2^-11):
  * rgb24 + trunc, finite inputs: bit-equal to torch.clamp(x, 0, 1).mul(255).to(torch.uint8) on the CPU (one float32 product);
  * everything else: nearest |b - v| <= 0.5 + delta; trunc v - 1 - delta < b <= v + delta.  The longest path (4:2:0 chroma) has 13
    float32 operations and 4 rounded constants, the + 0.5 one more; each is off by at most half an ulp of a magnitude below 256
    once scaled to the output, 2^-16 absolute, so 32 roundings are a safe ceiling: 32 * 2^-16 = 2^-11.  A float32 restatement of
    the formulas stays within 3.3e-5 (tests/test_frames_out_cpu.py checks that on these inputs), a wrong coefficient or order of
    steps moves bytes by whole fractions of a level;
  * on the noise and ramp images at most 2e-3 of the bytes differ from the exactly rounded float64 value (twice the width of the
    band in which delta allows either neighbour).  Not applied to frames of fewer than 500 bytes (2 x 2), where one byte in the
    band is already more than 2e-3 of the frame;
  * NaN and -inf give the byte of 0, +inf the byte of 1; two runs give identical bytes.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

from gsvc_amd import frames_out as fo
from gsvc_amd.frames_out import FrameFormat
from tests import _frames_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARE_CAP = 2e-3
SIZES = {(2, 2): 16, (34, 50): 8, (33, 47): 3, (270, 480): 3, (1080, 1920): 1}          # size -> images per launch in the big sweep
FORMATS = [(layout, matrix, rng, rounding) for layout in ("rgb24", "yuv444p", "yuv420p") for matrix in ("bt709", "bt601")
           for rng in ("limited", "full") for rounding in ("trunc", "nearest")]


def _inputs(n, H, W, first=0):
    """n seeded images cycling through noise / ramp / k over 255 / noise with NaN and inf pixels -> [(kind, float32 numpy)]"""
    return [(ref.KINDS[(first + k) % 4], ref.make_image(ref.KINDS[(first + k) % 4], H, W, seed=first + k)) for k in range(n)]


def _check_frame(got, kind, img, layout, matrix, rng, rounding, what):
    v = ref.values(img, layout, matrix, rng)
    bad, excess = ref.check_bytes(got, v, rounding)
    want = ref.quantise(v, rounding)
    share = float((got != want).mean())
    if os.environ.get("GSVC_PRINT_ERRORS"):
        print(f"{what} {kind}: outside the tolerance {bad}, worst excess {excess:.3e}, share differing from exact rounding {share:.3e}")
    assert bad == 0, (what, kind, bad, excess)
    if kind in ("noise", "ramp") and got.size >= 500:
        assert share <= SHARE_CAP, (what, kind, share)
    finite = np.isfinite(img).all()
    if layout == "rgb24" and rounding == "trunc" and finite:
        exact = torch.clamp(torch.from_numpy(img), 0, 1).mul(255).to(torch.uint8).permute(1, 2, 0).reshape(-1).numpy()
        assert np.array_equal(got, exact), (what, kind, int((got != exact).sum()))
    if not finite:          # NaN, -inf -> the byte of 0; +inf -> the byte of 1 (whole pixels in rgb24 / 4:4:4; 4:2:0 chroma mixes its block)
        H, W = img.shape[1:]
        fmt = FrameFormat(layout, matrix, rng, rounding)
        zero = ref.convert(np.zeros((3, 2, 2)), layout, matrix, rng, rounding)
        one = ref.convert(np.ones((3, 2, 2)), layout, matrix, rng, rounding)
        p = fo.planes(got, H, W, fmt)
        if layout == "rgb24":
            rgb = p[0].transpose(2, 0, 1)
            assert (rgb[np.isnan(img) | (img == -np.inf)] == 0).all() and (rgb[img == np.inf] == 255).all()
        else:
            low = (np.isnan(img) | (img == -np.inf)).all(axis=0)
            high = (img == np.inf).all(axis=0)
            assert H * W < 64 or (low.any() and high.any())
            assert (p[0][low] == zero[0]).all() and (np.abs(p[0][high].astype(int) - int(one[0])) <= (rounding == "trunc")).all()


@pytest.mark.parametrize("size", list(SIZES), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout,matrix,rng,rounding", FORMATS, ids=lambda x: x)
def test_kernel_against_float64(layout, matrix, rng, rounding, size):
    H, W = size
    if layout == "yuv420p" and (H % 2 or W % 2):
        with pytest.raises(ValueError, match="even"):
            fo.frames_to_u8([torch.zeros(3, H, W, device="cuda")], FrameFormat(layout, matrix, rng, rounding))
        return
    n = SIZES[size]
    fmt = FrameFormat(layout, matrix, rng, rounding)
    inputs = _inputs(n, H, W, first=(H + len(layout)) % 4)
    images = [torch.from_numpy(img).cuda() for _, img in inputs]          # separate allocations
    out = fo.frames_to_u8(images, fmt)
    again = fo.frames_to_u8(images, fmt)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (n, fo.frame_bytes(H, W, fmt))
    assert torch.equal(out, again)
    got = out.cpu().numpy()
    for k, (kind, img) in enumerate(inputs):
        _check_frame(got[k], kind, img, layout, matrix, rng, rounding, f"{layout} {matrix} {rng} {rounding} {H}x{W} [{k}]")


@pytest.mark.parametrize("n", [1, 3, 8, 16])
@pytest.mark.parametrize("layout", ["rgb24", "yuv444p", "yuv420p"])
def test_batch_sizes_strides_and_guard_bytes(layout, n):
    """n images in one launch into a buffer whose stride is larger than a frame: the bytes before, between and after the frames
    come back untouched, on the wide path (270 x 480) and on the edge path (34 x 50)."""
    fmt = FrameFormat(layout)
    for (H, W), pad in (((270, 480), 64), ((34, 50), 13), ((270, 480), 13)):          # (an odd stride: the edge path at a wide size)
        nb = fo.frame_bytes(H, W, fmt)
        inputs = _inputs(n, H, W, first=n)
        images = [torch.from_numpy(img).cuda() for _, img in inputs]
        lead = 32
        buf = torch.full((lead + n * (nb + pad) + 40,), 0xA5, dtype=torch.uint8, device="cuda")
        view = buf[lead:lead + n * (nb + pad)].view(n, nb + pad)
        ret = fo.frames_to_u8(images, fmt, out=view)
        assert ret.data_ptr() == view.data_ptr() and tuple(ret.shape) == (n, nb)
        host = buf.cpu().numpy()
        assert (host[:lead] == 0xA5).all() and (host[lead + n * (nb + pad):] == 0xA5).all()
        rows = host[lead:lead + n * (nb + pad)].reshape(n, nb + pad)
        assert (rows[:, nb:] == 0xA5).all()
        plain = fo.frames_to_u8(images, fmt).cpu().numpy()
        assert np.array_equal(rows[:, :nb], plain)          # the same bytes whichever path and stride
        for k, (kind, img) in enumerate(inputs):
            _check_frame(rows[k, :nb], kind, img, layout, "bt709", "limited", fmt.rounding_used, f"{layout} n={n} {H}x{W} pad {pad} [{k}]")


@pytest.mark.parametrize("layout", ["rgb24", "yuv444p", "yuv420p"])
def test_1080p_batch_of_eight(layout):
    H, W = 1080, 1920
    fmt = FrameFormat(layout)
    inputs = _inputs(8, H, W, first=1)
    out = fo.frames_to_u8([torch.from_numpy(img).cuda() for _, img in inputs], fmt).cpu().numpy()
    for k, (kind, img) in enumerate(inputs):
        _check_frame(out[k], kind, img, layout, "bt709", "limited", fmt.rounding_used, f"{layout} 1080p [{k}]")


@pytest.mark.parametrize("layout", ["rgb24", "yuv444p", "yuv420p"])
@pytest.mark.parametrize("size", [(34, 50), (270, 480)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_views_at_a_base_that_is_4_but_not_16_byte_aligned(layout, size):
    H, W = size
    fmt = FrameFormat(layout)
    inputs = _inputs(3, H, W, first=2)
    px = 3 * H * W
    pool = torch.zeros(3 * (px + 7) + 8, dtype=torch.float32, device="cuda")
    views = []
    for k, (_, img) in enumerate(inputs):
        at = k * (px + 7) + 1 + k          # 4, 40, ... bytes past a 16-byte boundary, never on one
        v = pool[at:at + px].view(3, H, W)
        v.copy_(torch.from_numpy(img))
        assert v.data_ptr() % 16 != 0 and v.data_ptr() % 4 == 0 and v.is_contiguous()
        views.append(v)
    got = fo.frames_to_u8(views, fmt).cpu().numpy()
    aligned = fo.frames_to_u8([torch.from_numpy(img).cuda() for _, img in inputs], fmt).cpu().numpy()
    assert np.array_equal(got, aligned)
    for k, (kind, img) in enumerate(inputs):
        _check_frame(got[k], kind, img, layout, "bt709", "limited", fmt.rounding_used, f"{layout} unaligned {H}x{W} [{k}]")


def test_non_contiguous_images_a_4d_tensor_and_more_than_one_launch():
    H, W = 34, 48
    fmt = FrameFormat("yuv420p")
    inputs = _inputs(20, H, W)
    stack = torch.from_numpy(np.stack([img for _, img in inputs])).cuda()
    want = np.stack([ref.convert(img, "yuv420p") for _, img in inputs])
    got = fo.frames_to_u8(stack, fmt).cpu().numpy()          # 20 images: two launches
    assert got.shape == want.shape and (np.abs(got.astype(int) - want.astype(int)) <= 1).all()
    transposed = [torch.from_numpy(np.ascontiguousarray(img.transpose(0, 2, 1))).cuda().permute(0, 2, 1) for _, img in inputs[:3]]
    assert not transposed[0].is_contiguous()
    assert np.array_equal(fo.frames_to_u8(transposed, fmt).cpu().numpy(), got[:3])
    with pytest.raises(ValueError, match="one size"):
        fo.frames_to_u8([stack[0], stack[1, :, :32]], fmt)
    with pytest.raises(ValueError, match="float32"):
        fo.frames_to_u8([stack[0].half()], fmt)


def test_launch_on_a_non_default_stream():
    H, W = 270, 480
    inputs = _inputs(3, H, W)
    images = [torch.from_numpy(img).cuda() for _, img in inputs]
    want = fo.frames_to_u8(images, FrameFormat("yuv420p"))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = fo.frames_to_u8(images, FrameFormat("yuv420p"))
    s.synchronize()
    assert torch.equal(got, want)


# ---- the decoder loop ---------------------------------------------------------------------------------------------------------
def _fitted(H, W, steps=6):
    from tests.test_train_gpu import _setup
    pc, cube, opt, pipe, mp, Trainer = _setup(anchors=4000, H=H, W=W)
    opt.full_precision_training_total = 1000
    pc.training_setup(opt)
    tr = Trainer(pc, cube, opt, pipe, mp)
    for it in range(1, steps + 1):          # a few fitting steps, so that the frames are not flat
        tr.step(it)
    return pc, cube, pipe


@pytest.mark.parametrize("size", [(96, 160), (192, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_render_frames_u8_equals_conversion_of_render_frames(size, tmp_path):
    from gsvc_amd.ortho_gaussian_renderer import render_frames
    H, W = size
    pc, cube, pipe = _fitted(H, W)
    bg = torch.zeros(3)
    for layout in ("rgb24", "yuv420p"):
        fmt = FrameFormat(layout)
        nb = fo.frame_bytes(H, W, fmt)
        for batch, count in ((1, 3), (3, 7), (8, 10), (8, 5), (3, 6)):          # not a multiple of the batch; fewer than one batch; a multiple
            frames = [cube.get_dummy_frame(i) for i in range(1, 1 + count)]
            floats = list(render_frames(frames, pc, pipe, bg, batch=batch))
            want = fo.frames_to_u8(floats, fmt)
            assert float(want.float().std()) > 1.0          # not flat
            on_dev = list(fo.render_frames_u8(frames, pc, pipe, bg, fmt=fmt, batch=batch, to_host=False))
            assert len(on_dev) == count and all(f.is_cuda and tuple(f.shape) == (nb,) for f in on_dev)
            assert torch.equal(torch.stack(on_dev), want)
            on_host = []
            for f in fo.render_frames_u8(frames, pc, pipe, bg, fmt=fmt, batch=batch, to_host=True):
                assert not f.is_cuda and f.dtype == torch.uint8 and tuple(f.shape) == (nb,)
                on_host.append(f.clone())          # cloned as they arrive: a frame is valid until the generator is advanced
            assert len(on_host) == count
            assert torch.equal(torch.stack(on_host), want.cpu()), (layout, batch, count)
    # write_video into a Y4M file gives those frames
    frames = [cube.get_dummy_frame(i) for i in range(0, 11)]
    fmt = FrameFormat("yuv420p")
    want = fo.frames_to_u8(list(render_frames(frames, pc, pipe, bg, batch=4)), fmt).cpu().numpy()
    path = tmp_path / "out.y4m"
    res = fo.write_video(frames, pc, pipe, bg, fo.Y4MWriter(path, W, H, fps=(24, 1), fmt=fmt), fmt=fmt, batch=4)
    hdr, back = fo.read_y4m(path)
    assert (hdr["W"], hdr["H"], hdr["fps"], hdr["layout"], hdr["range"]) == (W, H, (24, 1), "yuv420p", "limited")
    assert np.array_equal(back, want)
    assert res["frames"] == 11 and res["bytes"] == os.path.getsize(path) and res["fps"] > 0 and res["seconds"] > 0
    assert list(fo.render_frames_u8([], pc, pipe, bg)) == []


def test_evaluate_eight_bit():
    from gsvc_amd.loss_utils import l1_loss_func, psnr_func, ssim_func
    from gsvc_amd.ortho_gaussian_renderer import render_frames
    from gsvc_amd.report import evaluate
    H, W = 192, 256
    pc, cube, pipe = _fitted(H, W, steps=8)
    bg = torch.zeros(3)
    ids = list(range(2, 8))
    plain = evaluate(pc, cube, pipe, bg, frame_ids=ids)
    assert sorted(plain) == ["fps", "frames", "l1", "lpips", "msssim", "psnr", "ssim"]          # today's keys, nothing more
    frames = [cube[i] for i in ids]
    floats = [torch.clamp(img, 0.0, 1.0) for img in render_frames(frames, pc, pipe, bg, batch=8)]
    gts = [torch.clamp(fr.image.cuda(), 0.0, 1.0).permute(0, 2, 1).contiguous() for fr in frames]
    assert plain["psnr"] == sum(float(psnr_func(a, b)) for a, b in zip(floats, gts)) / len(ids)
    ev = evaluate(pc, cube, pipe, bg, frame_ids=ids, eight_bit=True)
    assert ev["eight_bit"] is True and sorted(set(ev) - {"eight_bit"}) == sorted(plain)
    u8 = fo.frames_to_u8(floats, FrameFormat("rgb24", rounding="trunc"))
    imgs = [(u8[k].view(H, W, 3).permute(2, 0, 1).float() / 255).contiguous() for k in range(len(ids))]
    assert ev["psnr"] == sum(float(psnr_func(a, b)) for a, b in zip(imgs, gts)) / len(ids)
    assert ev["ssim"] == sum(float(ssim_func(a, b).mean()) for a, b in zip(imgs, gts)) / len(ids)
    assert ev["l1"] == sum(float(l1_loss_func(a, b).mean()) for a, b in zip(imgs, gts)) / len(ids)
    assert ev["psnr"] != plain["psnr"] and abs(ev["psnr"] - plain["psnr"]) < 0.5          # 8 bits move it, and not far


def test_fit_tool_writes_the_decoded_video(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fit_synthetic
    out, video = tmp_path / "rd.json", tmp_path / "decoded.y4m"
    H, W, T = 272, 480, 24          # (the size of tests/test_fit_tool_gpu.py)
    fit_synthetic.main(["--steps", "80", "--height", str(H), "--width", str(W), "--frames", str(T), "--anchors", "8000", "--eval-frames", "4",
                        "--slab-frames", "8", "--payload-tol", "0.5", "--json", str(out), "--write-decoded", str(video)])
    log = json.loads(out.read_text())
    dv = log["decoded_video"]
    assert dv["frames"] == T and dv["layout"] == "yuv420p" and dv["fps"] > 0
    hdr, frames = fo.read_y4m(video)
    assert (hdr["W"], hdr["H"], hdr["layout"]) == (W, H, "yuv420p")
    assert frames.shape == (T, H * W * 3 // 2) and dv["bytes"] == os.path.getsize(video)
    assert frames[:, :H * W].std() > 1.0          # a picture, not a flat field
