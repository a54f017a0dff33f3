"""MS-SSIM as a fitting loss, without a GPU: the float64 restatement of tests/_msssim_loss_ref.py against ``metrics.ms_ssim``, the
backward formula of csrc/msssim_loss.hip written out by hand against float64 autograd, the CPU path of ``ms_ssim_l1`` (plain and
with ``img_b``), the ``distortion`` switch of the step and of the tools, and the host-side checks of the C entries."""
import ctypes as C
import os
import sys

import pytest
import torch

from tests import _msssim_loss_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("H,W,P", mr.SHAPES, ids=mr.SHAPE_IDS)
def test_restatement_is_metrics_ms_ssim(H, W, P):
    """metrics.ms_ssim casts to float32: it is the function, not the reference.  Bound 1e-5 (its float32 error; 6e-7 observed)."""
    from gsvc_amd.metrics import ms_ssim
    for sigma in mr.SIGMAS:
        x, y = mr.pictures(H, W, P, sigma)
        t = mr.ms_terms(x, y)
        assert float(t.min()) >= 0.64, (sigma, t)          # no plane of the test pictures is clipped by accident
        ref = float(mr.ms_ssim_l1(x, y)[0])
        got = float(ms_ssim(x.unsqueeze(0), y.unsqueeze(0), data_range=1))
        assert abs(got - ref) <= 1e-5, (sigma, got, ref)


@pytest.mark.parametrize("H,W,P", mr.SHAPES[:2], ids=mr.SHAPE_IDS[:2])
def test_backward_formula_is_float64_autograd(H, W, P):
    for sigma in mr.SIGMAS:
        x, y = mr.pictures(H, W, P, sigma)
        for g_ms, g_l1 in ((-0.2, 0.8), (1.0, 0.0)):
            want = mr.grad_autograd(x, y, g_ms, g_l1)
            got = mr.grad_by_hand(x, y, g_ms, g_l1)
            rel = float((got - want).abs().max() / want.abs().max())
            assert rel <= 1e-10, (sigma, g_ms, g_l1, rel)


def test_backward_formula_on_a_clipped_plane():
    """An anti-correlated pair: float64 autograd gives value 0 and gradient exactly 0, and so does the formula."""
    x, y = mr.pictures(161, 161, 1, 0.02)
    x = 1 - y
    assert float(mr.ms_terms(x, y).min()) < 0
    assert float(mr.ms_ssim_l1(x, y)[0]) == 0.0
    assert not mr.grad_autograd(x, y, 1.0, 0.0).any()
    assert not mr.grad_by_hand(x, y, 1.0, 0.0).any()


def test_cpu_path_is_the_restatement_and_differentiable():
    from gsvc_amd.loss_utils import ms_ssim_l1
    H, W, P = 161, 170, 2
    x, y = mr.pictures(H, W, P, 0.1)
    ref_ms, ref_l1 = mr.ms_ssim_l1(x, y)
    a = x.float().requires_grad_(True)
    ms, l1 = ms_ssim_l1(a, y.float())
    assert ms.dtype == torch.float32 and l1.dtype == torch.float32 and ms.dim() == 0
    assert abs(float(ms.detach()) - float(ref_ms)) <= 1e-5 and abs(float(l1.detach()) - float(ref_l1)) <= 1e-6
    (-0.2 * ms + 0.8 * l1).backward()
    want = mr.grad_autograd(x, y, -0.2, 0.8)
    assert torch.isfinite(a.grad).all() and float((a.grad.double() - want).abs().max() / want.abs().max()) < 1e-2
    # the pair form: the two-view frame formed by tensor expressions, gradients to both views
    f = x.float().requires_grad_(True)
    b = torch.flip(x.float(), dims=[2]).requires_grad_(True)
    ms2, l12, avg = ms_ssim_l1(f, y.float(), img_b=b)
    assert not avg.requires_grad and torch.equal(avg, x.float())
    assert torch.equal(ms2.detach(), ms.detach()) and torch.equal(l12.detach(), l1.detach())
    (-0.2 * ms2 + 0.8 * l12).backward()
    assert torch.allclose(f.grad, 0.5 * a.grad, rtol=0, atol=1e-12) and torch.equal(b.grad, torch.flip(f.grad, dims=[2]))
    with pytest.raises(ValueError):
        ms_ssim_l1(torch.zeros(3, 160, 200), torch.zeros(3, 160, 200))
    with pytest.raises(ValueError, match="one shape"):
        ms_ssim_l1(torch.zeros(3, 170, 200), torch.zeros(1, 170, 200))


# ------------------------------------------------------------------------------------------------ the switch
class _Cube:
    """What Trainer.__init__ reads of a dataset before it refuses a distortion."""
    len_z_frames = 4

    def __init__(self, H, W):
        self.height, self.width = H, W


def _trainer(cube, distortion, domain="rgb"):
    from gsvc_amd.arguments import OptimizationParams
    from gsvc_amd.train import Trainer
    opt = OptimizationParams()
    opt.distortion, opt.loss_domain = distortion, domain
    return Trainer(None, cube, opt, None, None)


def test_default_distortion_is_ssim():
    from gsvc_amd.arguments import OptimizationParams, cfg_20240919
    from gsvc_amd.encode_options import EncodeOptions
    assert OptimizationParams().distortion == "ssim"
    assert cfg_20240919()[1].distortion == "ssim"
    assert EncodeOptions().distortion == "ssim"


def test_trainer_refusals():
    with pytest.raises(ValueError, match="unknown distortion 'ssim3'"):
        _trainer(_Cube(176, 192), "ssim3")
    for domain in ("yuv420", "yuv444"):
        with pytest.raises(ValueError, match="loss_domain must be 'rgb'"):
            _trainer(_Cube(176, 192), "ms_ssim", domain)
    for H, W in ((160, 192), (176, 160), (96, 64)):
        with pytest.raises(ValueError, match="sides above 160"):
            _trainer(_Cube(H, W), "ms_ssim")


@pytest.mark.parametrize("tool", ["gsvc_encode", "fit_synthetic"])
def test_tools_parse_distortion(tool, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    mod = __import__(tool)
    base = ["clip.y4m", "-o", "clip.gsvc"] if tool == "gsvc_encode" else []
    with pytest.raises(SystemExit) as e:
        mod.main(base + ["--distortion", "psnr"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--distortion" in err and "ms_ssim" in err
    # both names are accepted: the parser gets past them to a check that runs after parsing
    for name in ("ssim", "ms_ssim"):
        with pytest.raises(SystemExit) as e:
            mod.main(base + ["--distortion", name, "--init-cell", "4"])
        assert e.value.code == 2
        err = capsys.readouterr().err
        assert "need --init detail" in err and "invalid choice" not in err


# ------------------------------------------------------------------------------------------------ the C entries, host side
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "gsvc_amd", "csrc", "libgsvc_hip.so")):
        g.build()
    from gsvc_amd import _lib
    return _lib.lib()


def test_workspace_bytes(lib):
    for P, H, W in ((1, 160, 400), (1, 400, 160), (0, 400, 400), (65536, 400, 400), (1, 32769, 400), (1, 64, 64)):
        assert lib.gsvc_msssim_loss_workspace_bytes(P, H, W) == -1, (P, H, W)
    small, big = lib.gsvc_msssim_loss_workspace_bytes(1, 161, 161), lib.gsvc_msssim_loss_workspace_bytes(3, 1080, 1920)
    assert 0 < small < big
    # three maps over the valid outputs of scale 0 alone
    assert big >= 3 * 3 * 1070 * 1910 * 4 and big % 256 == 0
    # it holds what gsvc_msssim's workspace holds of pooled pictures, and more
    assert big > lib.gsvc_msssim_workspace_bytes(3, 1080, 1920)


def test_entries_refuse_before_any_gpu_call(lib):
    buf = (C.c_float * 64)()
    p = C.addressof(buf) + 64
    p -= p % 16                                            # a 16-byte aligned address inside the buffer; no call below gets past the checks
    good = dict(img=p, img_b=None, gt=p, P=3, H=176, W=192, ws=p, out=p, avg=None, grads=p, d=p, db=None)

    def fwd(**kw):
        a = {**good, **kw}
        return lib.gsvc_msssim_loss_forward(a["img"], a["img_b"], a["gt"], a["P"], a["H"], a["W"], 1, a["ws"], a["out"], a["avg"], None)

    def bwd(**kw):
        a = {**good, **kw}
        return lib.gsvc_msssim_loss_backward(a["img"], a["img_b"], a["gt"], a["P"], a["H"], a["W"], a["ws"], a["grads"], a["d"], a["db"], None)

    def refused(rc, who, text):
        assert rc != 0
        msg = lib.gsvc_last_error().decode()
        assert msg.startswith(who + ":") and text in msg, msg

    for call, who in ((fwd, "msssim_loss_forward"), (bwd, "msssim_loss_backward")):
        refused(call(img=None), who, "NULL pointer")
        refused(call(gt=None), who, "NULL pointer")
        refused(call(ws=None), who, "NULL pointer")
        refused(call(P=0), who, "P must be 1 .. 65535")
        refused(call(P=65536), who, "P must be 1 .. 65535")
        refused(call(H=160), who, "exceed 160 pixels")
        refused(call(W=160), who, "exceed 160 pixels")
        refused(call(H=40000), who, "1 .. 32768")
        refused(call(img=p + 2), who, "4-byte aligned")
        refused(call(ws=p + 8), who, "16-byte aligned")
    refused(fwd(out=None), "msssim_loss_forward", "NULL pointer")
    refused(fwd(avg=p), "msssim_loss_forward", "avg_out without img_b")
    refused(bwd(grads=None), "msssim_loss_backward", "NULL pointer")
    refused(bwd(d=None), "msssim_loss_backward", "NULL pointer")
    refused(bwd(img_b=p), "msssim_loss_backward", "go together")
    refused(bwd(db=p), "msssim_loss_backward", "go together")
