#!/usr/bin/env python3
"""Two questions about a fit in the Y'CbCr loss domain, on the 1080p synthetic video written as yuv420p:
(a) do the file's own planes agree with the transform of its RGB pictures, in every frame and for both residencies;
(b) after the 500 full-precision steps of the 2 000-step schedule, per loss domain: PSNR of the render's luma and chroma planes against
    the file's planes, of the clamped render too, and how far the render leaves [0, 1].
One JSON document (``--json``); recorded in profiles/yuv_loss_gain.json.

    python tools/ab/yuv_domain_probe.py [--json out.json]
"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench_yuv_loss  # noqa: E402
from gsvc_amd import yuv_loss  # noqa: E402
from gsvc_amd.arguments import cfg_20240919  # noqa: E402
from gsvc_amd.fit_setup import configure_fit, new_fit  # noqa: E402
from gsvc_amd.frames_in import VideoFileCube  # noqa: E402
from gsvc_amd.generate import GenerateMode  # noqa: E402
from gsvc_amd.ortho_gaussian_renderer import render_pair  # noqa: E402


def psnr(a, b):
    return float(10 * torch.log10(1.0 / torch.mean((a - b) ** 2)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("yuv_domain_probe.py runs on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    H, W, T = 1080, 1920, 64
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "synth.y4m")
        bench_yuv_loss.write_clip(path, H, W, T, dev, seed=1234)
        for resident in ("float", "u8"):
            cube = VideoFileCube(path, resident=resident, device=dev)
            worst_y = worst_c = 0.0
            for i in range(T):
                tY, tC = yuv_loss.target_planes(cube, i, "yuv420p", "bt709")
                with torch.no_grad():
                    Y, C, _ = yuv_loss.yuv_planes(cube[i].image.permute(0, 2, 1).contiguous(), None, "yuv420p", "bt709")
                worst_y, worst_c = max(worst_y, float((Y - tY).abs().max())), max(worst_c, float((C - tC).abs().max()))
            out[f"native_vs_rgb_transform_{resident}"] = {"max_abs_luma": worst_y, "max_abs_chroma": worst_c}
            del cube
        for domain in ("yuv420", "rgb"):
            cube = VideoFileCube(path, resident="float", device=dev)
            mp_, opt, pipe = cfg_20240919()
            opt.optical_lambda = 0.0
            configure_fit(mp_, opt, cube, 2000, 0.004, 16.0, None)
            opt.loss_domain = domain
            pc, trainer = new_fit(cube, mp_, opt, pipe, 100_000, dev)
            for it in range(1, 501):          # the full-precision phase only
                step = trainer.step(it)
            rows = []
            with torch.no_grad():
                for i in (5, 20, 33, 50):
                    img = render_pair(cube[i], pc, pipe, trainer.background, mode=GenerateMode.TRAINING_FULL_PRECISION).rendered_image
                    tY, tC = yuv_loss.target_planes(cube, i, "yuv420p", "bt709")
                    Y, C, _ = yuv_loss.yuv_planes(img.contiguous(), None, "yuv420p", "bt709")
                    Yc, Cc, _ = yuv_loss.yuv_planes(img.clamp(0, 1).contiguous(), None, "yuv420p", "bt709")
                    gt = cube[i].image.permute(0, 2, 1)
                    rows.append({"frame": i, "psnr_y_unclamped": psnr(Y, tY), "psnr_y_clamped": psnr(Yc, tY), "psnr_c_unclamped": psnr(C, tC),
                                 "psnr_c_clamped": psnr(Cc, tC), "psnr_rgb_unclamped": psnr(img, gt), "psnr_rgb_clamped": psnr(img.clamp(0, 1), gt),
                                 "rgb_min": float(img.min()), "rgb_max": float(img.max()), "share_outside_01": float(((img < 0) | (img > 1)).float().mean()),
                                 "mean_abs_rgb_err_per_channel": [float(v) for v in (img - gt).abs().mean(dim=(1, 2))], "loss": float(step.loss)})
            out[f"after_500_steps_{domain}"] = rows
            trainer.close()
            del trainer, pc, cube
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
