"""MS-SSIM as a fitting loss on the GPU: ``ms_ssim_l1``, plain and with ``img_b`` (csrc/msssim_loss.hip), against the float64 restatement of
tests/_msssim_loss_ref.py, the step with ``distortion = "ms_ssim"``, and tools/gsvc_encode.py --distortion ms_ssim.

Error rule: the kernels' error against float64 is at most TWICE the error of the same function as float32 tensor expressions
(``_msssim_loss_ref`` run in float32 on the same GPU tensors, measured in the test) — twice, because the two sum in different orders.
Value: |MS-SSIM - ref|.  Gradient: max|g - g64| / max|g64| with upstream weights (-0.2, 0.8), the signs and sizes the step uses.  The
float64 reference is taken on the float32 pictures themselves (their exact float64 values).  Exact compares wherever the result must
not depend on rounding: the L1 gradient, a clipped plane, the pair form against the plain form, two runs.  GSVC_PRINT_ERRORS=1 prints
the figures of every case."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _msssim_loss_ref as mr
from tests._loss_kernel_refs import PRINT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G_MS, G_L1 = -0.2, 0.8
CASES = [(H, W, P, s) for H, W, P in mr.SHAPES for s in mr.SIGMAS]
CASE_IDS = [f"{i}-s{s}" for i in mr.SHAPE_IDS for s in mr.SIGMAS]


def _same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def _refs(x, y, g_ms=G_MS, g_l1=G_L1):
    """float32 [P, H, W] CUDA pictures -> the float64 value, L1 and gradient, and the errors of the float32 tensor expressions."""
    xd, yd = x.double(), y.double()
    ms64, l164 = (float(v) for v in mr.ms_ssim_l1(xd, yd))
    g64 = mr.grad_autograd(xd, yd, g_ms, g_l1)
    ms32 = float(mr.ms_ssim_l1(x, y)[0])
    g32 = mr.grad_autograd(x, y, g_ms, g_l1)
    scale = float(g64.abs().max())
    return {"ms": ms64, "l1": l164, "grad": g64, "scale": scale, "e32_value": abs(ms32 - ms64),
            "e32_grad": float((g32.double() - g64).abs().max()) / scale}


@functools.lru_cache(maxsize=None)
def _case(H, W, P, sigma):
    x, y = (t.float().cuda() for t in mr.pictures(H, W, P, sigma))
    return x, y, _refs(x, y)


def _loss_and_grad(x, y, g_ms=G_MS, g_l1=G_L1):
    from gsvc_amd.loss_utils import ms_ssim_l1
    a = x.clone().requires_grad_(True)
    ms, l1 = ms_ssim_l1(a, y)
    (g_ms * ms + g_l1 * l1).backward()
    return ms.detach(), l1.detach(), a.grad


@pytest.mark.parametrize("H,W,P,sigma", CASES, ids=CASE_IDS)
def test_value_and_gradient(H, W, P, sigma):
    x, y, ref = _case(H, W, P, sigma)
    ms, l1, g = _loss_and_grad(x, y)
    assert ms.dtype == torch.float32 and l1.dtype == torch.float32 and g.dtype == torch.float32 and g.shape == x.shape
    e_value = abs(float(ms.double()) - ref["ms"])
    e_grad = float((g.double() - ref["grad"]).abs().max()) / ref["scale"]
    figures = (f"value error {e_value:.3e} (float32 expressions {ref['e32_value']:.3e}), "
               f"gradient error {e_grad:.3e} (float32 autograd {ref['e32_grad']:.3e})")
    if PRINT:
        print(f"MSSSIM_LOSS {H}x{W}x{P} sigma {sigma}: {figures}")
    assert torch.isfinite(g).all()
    assert abs(float(l1.double()) - ref["l1"]) <= 1e-6 * ref["l1"], (float(l1), ref["l1"])
    assert e_value <= 2 * ref["e32_value"], figures
    assert e_grad <= 2 * ref["e32_grad"], figures


@pytest.mark.parametrize("H,W,P", mr.SHAPES, ids=mr.SHAPE_IDS)
def test_l1_gradient_is_exact(H, W, P):
    """Upstream (0, 0.8): every pixel gets 0.8 / (P H W) * sign(x - y), one float32 division, whoever owns it."""
    x, y, _ = _case(H, W, P, 0.1)
    _, _, g = _loss_and_grad(x, y, 0.0, G_L1)
    step = torch.tensor(G_L1, dtype=torch.float32, device="cuda") / torch.tensor(float(P * H * W), dtype=torch.float32, device="cuda")
    want = step * torch.sign(x - y)
    assert bool((torch.sign(x - y) == 0).any()) and bool((torch.sign(x - y) != 0).any())      # clamped pixels are ties
    assert torch.equal(g, want)


def test_clipped_plane():
    from gsvc_amd.loss_utils import ms_ssim_l1
    H, W = 176, 208
    x, y, _ = _case(H, W, 2, 0.02)
    x = torch.stack([x[0], 1 - y[1]])
    ref = _refs(x, y, G_MS, 0.0)
    assert float(mr.ms_terms(x.double(), y.double())[:, 1].min()) < 0
    alone = ms_ssim_l1(x[1:], y[1:])[0]
    assert float(alone) == 0.0
    ms, l1, g = _loss_and_grad(x, y, G_MS, 0.0)
    assert np.isfinite(float(ms)) and np.isfinite(float(l1)) and torch.isfinite(g).all()
    assert not g[1].any(), "the clipped plane's MS-SSIM gradient is exactly 0"
    e_value = abs(float(ms.double()) - ref["ms"])
    e_grad = float((g[0].double() - ref["grad"][0]).abs().max()) / ref["scale"]
    figures = f"value {e_value:.3e} ({ref['e32_value']:.3e}), gradient {e_grad:.3e} ({ref['e32_grad']:.3e})"
    assert e_value <= 2 * ref["e32_value"] and e_grad <= 2 * ref["e32_grad"], figures
    # with the L1 term on, the clipped plane carries the L1 gradient alone
    _, _, g2 = _loss_and_grad(x, y)
    step = torch.tensor(G_L1, dtype=torch.float32, device="cuda") / torch.tensor(float(2 * H * W), dtype=torch.float32, device="cuda")
    assert torch.isfinite(g2).all() and torch.equal(g2[1], step * torch.sign(x[1] - y[1]))


@pytest.mark.parametrize("H,W,P", [mr.SHAPES[1], mr.SHAPES[3]], ids=[mr.SHAPE_IDS[1], mr.SHAPE_IDS[3]])
def test_pair_form_is_the_plain_form_of_the_averaged_frame(H, W, P):
    from gsvc_amd.loss_utils import ms_ssim_l1
    f, gt, _ = _case(H, W, P, 0.1)
    b = _case(H, W, P, 0.02)[0].roll(3, dims=2)
    avg_t = 0.5 * (f + torch.flip(b, dims=[2]))
    ms, l1, g = _loss_and_grad(avg_t, gt)
    ff, bb = f.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ms_p, l1_p, avg = ms_ssim_l1(ff, gt, img_b=bb)
    assert not avg.requires_grad
    (G_MS * ms_p + G_L1 * l1_p).backward()
    assert _same_bits(avg, avg_t) and _same_bits(ms_p.detach(), ms) and _same_bits(l1_p.detach(), l1)
    assert _same_bits(ff.grad, 0.5 * g)
    assert _same_bits(bb.grad, torch.flip(ff.grad, dims=[2]))


def test_two_runs_give_the_same_bits():
    x, y, _ = _case(170, 202, 3, 0.1)
    first, second = _loss_and_grad(x, y), _loss_and_grad(x, y)
    for a, b in zip(first, second):
        assert _same_bits(a, b)


# ------------------------------------------------------------------------------------------------ the step
H_, W_, T_ = 176, 192, 4


def _fit(cube, distortion, batched):
    from gsvc_amd.arguments import cfg_20240919
    from gsvc_amd.fit_setup import configure_fit, new_fit
    from gsvc_amd.train import Trainer
    mp_, opt, pipe = cfg_20240919()
    opt.optical_lambda = 0.0
    configure_fit(mp_, opt, cube, 100, 0.004, 8.0, 2e-5)
    opt.distortion = distortion
    pc, trainer = new_fit(cube, mp_, opt, pipe, 2000, torch.device("cuda", 0))
    if not batched:
        trainer.close()
        trainer = Trainer(pc, cube, opt, pipe, mp_, seed=0, batched=False)
    return opt, pc, trainer


def _watch_gradients(pc):
    """{(group name, index): finite} of every parameter that holds a gradient when the optimizer steps."""
    seen = {}
    real = pc.optimizer.step

    def step(*args, **kwargs):
        for group in pc.optimizer.param_groups:
            for i, p in enumerate(group["params"]):
                if p.grad is not None:
                    key = (group.get("name"), i)
                    seen[key] = seen.get(key, True) and bool(torch.isfinite(p.grad).all())
        return real(*args, **kwargs)
    pc.optimizer.step = step
    return seen


@pytest.mark.parametrize("batched", [True, False], ids=["batched", "unbatched"])
def test_step_with_ms_ssim(batched):
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.loss_utils import render_regs
    from gsvc_amd.train import _mean_over_selected
    from gsvc_amd.yuv_loss import distortion_weights
    cube = SyntheticFrameCube(H_, W_, T_, seed=7, device="cuda").materialize()
    grads = {}
    for distortion in ("ssim", "ms_ssim"):
        opt, pc, trainer = _fit(cube, distortion, batched)
        assert trainer.distortion == distortion
        seen = _watch_gradients(pc)
        out = trainer.step(1, frame_idx=2)
        torch.cuda.synchronize()
        if distortion == "ms_ssim":
            assert not trainer.controller.entropy_constrained          # (step 1 is full precision: no rate term)
            r1f, r1b, r2f, r2b = out.renders
            with torch.no_grad():
                image_terms = []
                for image, i in ((out.image1, 2), (out.image2, 3)):
                    gt = cube[i].image.cuda().permute(0, 2, 1).contiguous()
                    image_terms.append(mr.ms_ssim_l1(image.double(), gt.double()))
                if batched:
                    batch = r1f.generated_gaussians.batch
                    regs = render_regs(batch.scaling, batch.neural_opacity, batch.mask, batch.seg_offsets)
                else:
                    regs = (sum(_mean_over_selected(r.scaling.prod(dim=1), r) for r in out.renders),
                            sum((1 - r.neural_opacity).mean() for r in out.renders))
            # D = (1 - l) L1 + l (1 - MS-SSIM) per frame, and that is what the step's weights say
            lam = opt.lambda_dssim
            assert distortion_weights("rgb", lam) == ([1.0 - lam] * 2 + [-lam] * 2, 2.0 * lam)
            by_hand = sum((1 - lam) * float(l1) + lam * (1 - float(ms)) for ms, l1 in image_terms)
            by_hand += opt.scaling_reg * float(regs[0]) + opt.opacity_reg * float(regs[1])
            assert np.isfinite(float(out.loss)) and abs(float(out.loss) - by_hand) <= 1e-5, (float(out.loss), by_hand)
        for it in (2, 3):
            assert np.isfinite(float(trainer.step(it).loss))
        trainer.close()
        grads[distortion] = seen
    assert grads["ssim"] and set(grads["ms_ssim"]) >= set(grads["ssim"])
    assert all(grads["ms_ssim"].values()), [k for k, ok in grads["ms_ssim"].items() if not ok]


def test_encode_with_ms_ssim_then_decode_in_another_process(tmp_path):
    """tools/gsvc_encode.py --distortion ms_ssim, then tools/gsvc_decode.py --strict in a fresh process: the distortion changes the fit,
    not the file format."""
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import FrameFormat, Y4MWriter, frames_to_u8
    clip, out, coded = str(tmp_path / "clip.y4m"), str(tmp_path / "out.y4m"), str(tmp_path / "clip.gsvc")
    cube = SyntheticFrameCube(H_, W_, T_, seed=7, device="cuda")
    fmt = FrameFormat("yuv420p")
    with Y4MWriter(clip, W_, H_, (25, 1), fmt) as sink:
        for fr in frames_to_u8([cube._image(t) for t in range(T_)], fmt).cpu():
            sink.write(fr)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gsvc_encode
    log = gsvc_encode.main([clip, "-o", coded, "--steps", "40", "--anchors", "2000", "--slab-frames", "8", "--densify-grad-threshold", "2e-5",
                            "--distortion", "ms_ssim"])
    assert log["distortion"] == "ms_ssim" and log["loss_domain"] == "rgb" and log["total_bytes"] == os.path.getsize(coded)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gsvc_decode.py"), coded, "-o", out, "--strict"], cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-2500:])
    line = json.loads(run.stdout.strip().splitlines()[-1])
    assert line["frames_verified"] == T_ and line["frames_mismatched"] == 0
