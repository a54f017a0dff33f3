"""The Y'CbCr loss domain without a GPU: the references of tests/_yuv_loss_ref.py pinned against the frame oracle of
tests/_frames_ref.py, the distortion weights, and everything that is refused before a kernel is launched."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _frames_ref as fr
from tests import _yuv_loss_ref as yr

SIZES = [(2, 2), (6, 10), (18, 34)]


def _picture(H, W, seed):
    """Float32 RGB strictly inside [0, 1]: the planes' transform has no clamp, the oracle clamps its inputs."""
    return np.random.default_rng(7000 + seed).uniform(0.02, 0.98, (3, H, W)).astype(np.float32)


# -------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("layout", ["yuv420p", "yuv444p"])
@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
@pytest.mark.parametrize("rng", ["limited", "full"])
def test_reference_planes_reproduce_the_frame_oracle(layout, matrix, rng):
    """planes -> clamp, range map, round = the codes of the delivered frame: the transform differs from frames_to_u8 by nothing else."""
    for k, (H, W) in enumerate(SIZES + ([(5, 7)] if layout == "yuv444p" else [])):
        img = _picture(H, W, k)
        v_oracle = fr.values(img, layout, matrix, rng)
        # away from rounding ties: the two float64 evaluations differ by ~1e-13, so a sample this far from k + 0.5 rounds alike in both
        tie = np.abs(v_oracle - np.floor(v_oracle) - 0.5)
        assert tie.min() > 1e-9, "the seeded picture has a sample on a rounding tie: change the seed"
        planes, _ = yr.planes_ref(torch.from_numpy(img).double(), None, layout, matrix)
        codes, v = yr.codes_of_planes(planes.numpy(), H, W, rng)
        assert np.abs(v - v_oracle).max() < 1e-10
        assert np.array_equal(codes.astype(np.uint8), fr.convert(img, layout, matrix, rng, "nearest"))


@pytest.mark.parametrize("layout,H,W", [("yuv420p", 6, 10), ("yuv444p", 5, 7)])
@pytest.mark.parametrize("pair", [False, True])
def test_reference_adjoint_is_the_transpose(layout, H, W, pair):
    """adjoint_ref (written from the header's formulas) against autograd through planes_ref, and <J x, y> = <x, J^T y> in float64."""
    gen = torch.Generator().manual_seed(11)
    f = torch.rand(3, H, W, generator=gen, dtype=torch.float64, requires_grad=True)
    b = torch.rand(3, H, W, generator=gen, dtype=torch.float64, requires_grad=True) if pair else None
    y = torch.randn(yr.plane_floats(H, W, layout), generator=gen, dtype=torch.float64)
    planes, _ = yr.planes_ref(f, b, layout, "bt709")
    grads = torch.autograd.grad((planes * y).sum(), (f, b) if pair else (f,))
    d_f, d_b = yr.adjoint_ref(y, H, W, layout, "bt709", pair)
    assert torch.allclose(d_f, grads[0], rtol=0, atol=1e-14)
    if pair:
        assert torch.allclose(d_b, grads[1], rtol=0, atol=1e-14)
    zero, _ = yr.planes_ref(torch.zeros_like(f), torch.zeros_like(f) if pair else None, layout, "bt709")
    lhs = ((planes - zero).detach() * y).sum()          # the transform is affine (chroma + 0.5): J x = planes(x) - planes(0)
    rhs = (f.detach() * d_f).sum() + ((b.detach() * d_b).sum() if pair else 0.0)
    assert abs(float(lhs - rhs)) < 1e-12 * float((planes.detach().abs() * y.abs()).sum())


@pytest.mark.parametrize("depth,rng", [(8, "limited"), (8, "full"), (10, "limited"), (16, "full")])
def test_reference_code_planes(depth, rng):
    """Black, white and the chroma zero land on 0, 1 and 0.5, and the map agrees with float64 to one rounding."""
    y_off, y_scale, c_off, c_scale, top = yr.range_constants(rng, depth)
    codes = np.array([y_off, y_off + y_scale, 0, top, c_off, c_off + c_scale / 2, 0, top], dtype=np.uint16)
    p = yr.code_planes_ref(codes, 2, 2, rng, depth)
    assert p[0] == 0.0 and p[1] == 1.0 and p[4] == 0.5
    ref = np.concatenate([(codes[:4].astype(np.float64) - y_off) / y_scale, (codes[4:].astype(np.float64) - c_off) / c_scale + 0.5])
    assert np.abs(p - ref).max() <= 2.0 ** -23 * max(1.0, np.abs(ref).max())


# -------------------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("lam", [0.2, 0.0, 0.35])
def test_distortion_weights(lam):
    from gsvc_amd.yuv_loss import distortion_weights
    w_rgb, c_rgb = distortion_weights("rgb", lam)
    assert w_rgb == [1.0 - lam] * 2 + [-lam] * 2 and c_rgb == 2.0 * lam          # today's step, unchanged
    for domain in ("yuv420", "yuv444"):
        w, c = distortion_weights(domain, lam)
        assert len(w) == 8                       # two frames x (L1, SSIM) x (luma, chroma)
        assert sum(w) == pytest.approx(sum(w_rgb), abs=1e-15) and c == pytest.approx(c_rgb, abs=1e-15)
        # per frame D = 0.75 D_Y + 0.25 D_C: a perfect fit (L1 0, SSIM 1) costs nothing, the worst L1 costs (1 - lam) per frame
        assert sum(w[4:]) + c == pytest.approx(0.0, abs=1e-15)
        assert w[0] == pytest.approx(3.0 * w[2]) and w[4] == pytest.approx(3.0 * w[6])


@pytest.mark.parametrize("domain", ["rgb", "yuv420", "yuv444"])
def test_interleaved_frame_terms_are_in_the_order_of_the_weights(domain):
    """A frame's tuple is its L1 terms, then its structural terms; the step interleaves the two frames' tuples.  That list is the one
    ``distortion_weights`` documents its weights for, name by name."""
    import re

    from gsvc_amd.loss_utils import StepDistortion
    from gsvc_amd.yuv_loss import distortion_weights
    documented = [re.split(r",\s*", m) for m in re.findall(r"``\[([^\]]+)\]``", distortion_weights.__doc__)]
    assert [len(d) for d in documented] == [4, 8]
    names = documented[0] if domain == "rgb" else documented[1]
    per_frame = ("l1_{}", "ssim_{}") if domain == "rgb" else ("l1_y{}", "l1_c{}", "ssim_y{}", "ssim_c{}")
    value = {n: 1.0 + 0.25 * k for k, n in enumerate(sorted(names))}          # a distinct constant per term
    frames = [tuple(value[n.format(k)] for n in per_frame) for k in (1, 2)]
    terms = StepDistortion.image_terms(*frames)
    assert terms == [value[n] for n in names]
    assert len(terms) == len(distortion_weights(domain, 0.2)[0])


def test_default_domain_is_rgb():
    from gsvc_amd.arguments import OptimizationParams, cfg_20240919
    assert OptimizationParams().loss_domain == "rgb"
    assert cfg_20240919()[1].loss_domain == "rgb"


# -------------------------------------------------------------------------------------------------- refusals
class _Cube:
    """What Trainer.__init__ reads of a dataset before it refuses a loss domain."""
    len_z_frames = 4

    def __init__(self, H, W, fmt=None, planes=False):
        self.height, self.width = H, W
        if fmt is not None:
            self.fmt = fmt
        if planes:
            self.yuv_planes = lambda i: None


def _trainer(cube, domain):
    from gsvc_amd.arguments import OptimizationParams
    from gsvc_amd.train import Trainer
    opt = OptimizationParams()
    opt.loss_domain = domain
    return Trainer(None, cube, opt, None, None)


def test_trainer_refuses_an_unknown_domain():
    with pytest.raises(ValueError, match="unknown loss_domain 'yuv422'"):
        _trainer(_Cube(48, 64), "yuv422")


@pytest.mark.parametrize("H,W", [(47, 64), (48, 63)])
def test_trainer_refuses_yuv420_on_odd_sizes(H, W):
    with pytest.raises(ValueError, match="needs even H and W"):
        _trainer(_Cube(H, W), "yuv420")


def test_yuv444_on_a_420_file_is_refused():
    from gsvc_amd.frames_out import FrameFormat
    from gsvc_amd.yuv_loss import target_planes
    cube = _Cube(48, 64, FrameFormat("yuv420p"), planes=True)
    with pytest.raises(ValueError, match="yuv444.*yuv420p file"):
        _trainer(cube, "yuv444")
    with pytest.raises(ValueError, match="yuv444.*yuv420p file"):
        target_planes(cube, 0, "yuv444p", "bt709")


class _Stub(_Cube):
    """A dataset that records what is asked of it; every sample it hands out has the value ``mark``."""

    def __init__(self, mark, H, W, fmt=None):
        super().__init__(H, W, fmt, planes=fmt is not None)
        self.mark, self.calls = float(mark), []
        if fmt is not None:
            self.yuv_planes = self._planes

    def __getitem__(self, i):
        self.calls.append(("item", i))
        return SimpleNamespace(image=torch.full((3, self.width, self.height), self.mark))      # (the cubes keep pictures transposed)

    def get_dummy_frame(self, i):
        self.calls.append(("dummy", i))
        return SimpleNamespace(image=None)

    def _planes(self, i):
        self.calls.append(("planes", i))
        return torch.full((self.height * self.width * 3 // 2,), self.mark)


@pytest.mark.parametrize("native", [False, True])
def test_the_step_distortion_reads_the_dataset_it_is_handed(native):
    """Built against stub A, it takes frame and target from stub B: the frame without its picture where the targets are the file's
    own planes, ``B[i]`` otherwise; and it keeps no dataset."""
    from gsvc_amd.arguments import OptimizationParams
    from gsvc_amd.frames_out import FrameFormat
    from gsvc_amd.loss_utils import StepDistortion
    H, W = 6, 10
    fmt = FrameFormat("yuv420p") if native else None
    a, b = _Stub(0.25, H, W, fmt), _Stub(0.75, H, W, fmt)
    opt = OptimizationParams()
    opt.loss_domain = "yuv420" if native else "rgb"
    dist = StepDistortion(opt, a)
    assert dist.native_planes == native and dist.layout == ("yuv420p" if native else None)
    a.calls.clear()
    frame = dist.frame(b, 2)
    target = dist.target(b, frame, 2, torch.device("cpu"))
    assert a.calls == []
    if native:
        assert b.calls == [("dummy", 2), ("planes", 2)]
        assert [tuple(t.shape) for t in target] == [(1, H, W), (2, H // 2, W // 2)] and all(bool((t == b.mark).all()) for t in target)
    else:
        assert b.calls == [("item", 2)]
        assert tuple(target.shape) == (3, H, W) and target.is_contiguous() and bool((target == b.mark).all())
    assert not any(isinstance(v, _Cube) for v in vars(dist).values())


def test_python_argument_checks():
    from gsvc_amd import yuv_loss
    from gsvc_amd.frames_out import FrameFormat
    assert yuv_loss.plane_shapes(6, 10, "yuv420p") == ((1, 6, 10), (2, 3, 5))
    assert yuv_loss.plane_shapes(5, 7, "yuv444p") == ((1, 5, 7), (2, 5, 7))
    with pytest.raises(ValueError, match="even H and W"):
        yuv_loss.plane_shapes(5, 8, "yuv420p")
    with pytest.raises(ValueError, match="not 'rgb24'"):
        yuv_loss.plane_shapes(4, 8, "rgb24")
    with pytest.raises(ValueError, match="unknown matrix"):
        yuv_loss.yuv_planes(torch.zeros(3, 4, 4), None, "yuv420p", "bt2020")
    # native planes: a Y'CbCr file of the requested layout only; the matrix is the file's, else BT.709
    assert yuv_loss.native_planes(_Cube(4, 4, FrameFormat("yuv420p"), planes=True), "yuv420p")
    assert not yuv_loss.native_planes(_Cube(4, 4, FrameFormat("yuv444p"), planes=True), "yuv420p")
    assert not yuv_loss.native_planes(_Cube(4, 4), "yuv420p")
    assert yuv_loss.loss_matrix(_Cube(4, 4, FrameFormat("yuv420p", "bt601"))) == "bt601"
    assert yuv_loss.loss_matrix(_Cube(4, 4, FrameFormat("rgb24", "bt601"))) == "bt709"
    assert yuv_loss.loss_matrix(_Cube(4, 4)) == "bt709"


def _refused(rc, text):
    from gsvc_amd import _lib
    assert rc != 0
    msg = _lib.lib().gsvc_last_error().decode()
    assert text in msg, msg


def test_entries_refuse_before_any_launch():
    """The argument checks of the three entries run on the host: their texts, with pointers that are never dereferenced."""
    from gsvc_amd import _lib
    L = _lib.lib()
    p = 0x1000
    ptrs = (C.c_void_p * 1)(p)
    L420, L444, RGB = yr.LAYOUT_ID["yuv420p"], yr.LAYOUT_ID["yuv444p"], yr.LAYOUT_ID["rgb24"]
    assert L.gsvc_yuv_planes_floats(6, 10, L420) == 90 and L.gsvc_yuv_planes_floats(5, 7, L444) == 105
    assert L.gsvc_yuv_planes_floats(5, 7, L420) < 0 and L.gsvc_yuv_planes_floats(4, 4, RGB) < 0
    _refused(L.gsvc_frames_planes(p, 96, 1, 8, 8, RGB, 0, 8, ptrs, None), "frames_planes: rgb24 frames hold no Y'CbCr planes")
    _refused(L.gsvc_frames_planes(p, 96, 0, 8, 8, L420, 0, 8, ptrs, None), "frames_planes: n must be 1 .. 16 (got 0)")
    _refused(L.gsvc_frames_planes(p, 96, 17, 8, 8, L420, 0, 8, ptrs, None), "frames_planes: n must be 1 .. 16 (got 17)")
    _refused(L.gsvc_frames_planes(p, 96, 1, 8, 8, L420, 0, 7, ptrs, None), "frames_planes: depth must be 8 .. 16 (got 7)")
    _refused(L.gsvc_frames_planes(p, 96, 1, 8, 8, L420, 0, 17, ptrs, None), "frames_planes: depth must be 8 .. 16 (got 17)")
    _refused(L.gsvc_frames_planes(p, 96, 1, 8, 8, L420, 2, 8, ptrs, None), "frames_planes: unknown range 2")
    _refused(L.gsvc_frames_planes(p, 96, 1, 7, 8, L420, 0, 8, ptrs, None), "frames_planes: yuv420p needs even H and W (got 7 x 8)")
    _refused(L.gsvc_frames_planes(p, 95, 1, 8, 8, L420, 0, 8, ptrs, None), "frames_planes: in_stride 95 is shorter than a frame (96 bytes)")
    _refused(L.gsvc_frames_planes(p + 1, 192, 1, 8, 8, L420, 0, 10, ptrs, None), "frames_planes: the frame base is not 2-byte aligned")
    _refused(L.gsvc_frames_planes(p, 193, 1, 8, 8, L420, 0, 10, ptrs, None), "frames_planes: in_stride 193 is not a multiple of 2")
    _refused(L.gsvc_frames_planes(p, 96, 1, 8, 8, L420, 0, 8, (C.c_void_p * 1)(p + 2), None), "frames_planes: image 0 is not 4-byte aligned")
    _refused(L.gsvc_frames_planes(None, 96, 1, 8, 8, L420, 0, 8, ptrs, None), "frames_planes: NULL pointer")
    _refused(L.gsvc_yuv_planes_forward(p, None, 8, 8, RGB, 0, p, None, None), "yuv_planes_forward: the layout must be yuv444p or yuv420p (got 0)")
    _refused(L.gsvc_yuv_planes_forward(p, None, 8, 7, L420, 0, p, None, None), "yuv_planes_forward: yuv420p needs even H and W (got 8 x 7)")
    _refused(L.gsvc_yuv_planes_forward(p, None, 8, 8, L420, 2, p, None, None), "yuv_planes_forward: unknown matrix 2")
    _refused(L.gsvc_yuv_planes_forward(p, None, 0, 8, L444, 0, p, None, None), "yuv_planes_forward: image size must be 1 .. 32768 (got 0 x 8)")
    _refused(L.gsvc_yuv_planes_forward(None, None, 8, 8, L420, 0, p, None, None), "yuv_planes_forward: NULL pointer")
    _refused(L.gsvc_yuv_planes_forward(p, p + 2, 8, 8, L420, 0, p, None, None), "yuv_planes_forward: img_b is not 4-byte aligned")
    _refused(L.gsvc_yuv_planes_backward(p, 8, 8, 5, 0, p, None, None), "yuv_planes_backward: the layout must be yuv444p or yuv420p (got 5)")
    _refused(L.gsvc_yuv_planes_backward(p, 9, 8, L420, 0, p, None, None), "yuv_planes_backward: yuv420p needs even H and W (got 9 x 8)")
    _refused(L.gsvc_yuv_planes_backward(p, 8, 8, L420, 0, None, None, None), "yuv_planes_backward: NULL pointer")
    _refused(L.gsvc_yuv_planes_backward(p, 8, 8, L420, 0, p, p + 1, None), "yuv_planes_backward: dL_dimg_b is not 4-byte aligned")
