#!/usr/bin/env python3
"""What fitting for MS-SSIM costs (csrc/msssim_loss.hip, gsvc_amd/loss_utils.py ms_ssim_l1).  One JSON line.

  loss      forward + backward of ``ms_ssim_l1`` at 1080 x 1920 x 3 against the same function as float32 tensor expressions
            (tests/_msssim_loss_ref.py) through autograd: device-event time of groups of 5 calls, the two alternated in one process,
            median over the groups; the pair form beside it.  Inputs rotate through enough sets to exceed the 256 MiB Infinity Cache.
  launches  each way: the library's kernel launches (``gsvc_profile_enable``) of one forward + backward, and the device kernels the
            tensor-expression form launches (torch.profiler).
  accuracy  the figures of tests/test_msssim_loss_gpu.py at 1080p, both sigmas: |value - float64|, max|g - g64| / max|g64| with upstream
            (-0.2, 0.8), for the kernels and for the float32 tensor expressions.
  step      a fitting step per distortion, the ``ssim`` and ``ms_ssim`` legs alternated in one process (two fits alive, groups of 10
            steps, median of the groups) on the 1080p synthetic video, 100 000 anchors, full-precision phase.  ``--ssim-step-only``
            measures the ``ssim`` leg alone with nothing this feature added: run on a checkout of the parent commit it is the
            baseline, handed back with ``--baseline``.

    python tools/bench_msssim_loss.py [--groups 20] [--step-frames 16] [--baseline parent.json] [--json profiles/msssim_loss.json]
    python tools/bench_msssim_loss.py --ssim-step-only --json parent.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gsvc_amd import _lib  # noqa: E402

CACHE = 300 << 20          # rotate through more than the 256 MiB last-level cache
H, W, P = 1080, 1920, 3
G_MS, G_L1 = -0.2, 0.8


def timed_group(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(calls):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls


def alternated(fns, groups, calls=5):
    for _ in range(2):
        for fn in fns.values():
            timed_group(fn, calls)
    times = {k: [] for k in fns}
    for _ in range(groups):
        for k, fn in fns.items():
            times[k].append(timed_group(fn, calls))
    return {k: {"us": 1e6 * statistics.median(v), "us_min_max": [1e6 * min(v), 1e6 * max(v)]} for k, v in times.items()}


def library_launches(fn):
    torch.cuda.synchronize()
    _lib.profile_enable(1)
    _lib.profile_collect(256)
    fn()
    torch.cuda.synchronize()
    counts = {k: v[0] for k, v in _lib.profile_collect(256).items()}
    _lib.profile_enable(0)
    return counts


def device_kernels(fn):
    """Device kernels one call of ``fn`` launches, as torch.profiler sees them (None where the profiler is not usable)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    except Exception:          # noqa: BLE001  (a profiler that cannot start is not a measurement)
        return None


def bench_loss(groups, dev):
    from gsvc_amd.loss_utils import ms_ssim_l1
    from tests import _msssim_loss_ref as mr
    sets = max(2, -(-CACHE // (3 * 4 * P * H * W)))
    ys = [mr.pictures(H, W, P, 0.1, seed=k)[1].float().to(dev) for k in range(sets)]
    xs = [(y + 0.05 * torch.randn_like(y)).clamp(0, 1).requires_grad_(True) for y in ys]
    bs = [x.detach().flip(-1).clone().requires_grad_(True) for x in xs]

    def fused(k):
        i = k % sets
        ms, l1 = ms_ssim_l1(xs[i], ys[i])
        torch.autograd.grad(G_MS * ms + G_L1 * l1, xs[i])

    def fused_pair(k):
        i = k % sets
        ms, l1, _ = ms_ssim_l1(xs[i], ys[i], img_b=bs[i])
        torch.autograd.grad(G_MS * ms + G_L1 * l1, (xs[i], bs[i]))

    def expressions(k):
        i = k % sets
        ms, l1 = mr.ms_ssim_l1(xs[i], ys[i])
        torch.autograd.grad(G_MS * ms + G_L1 * l1, xs[i])
    res = {"H": H, "W": W, "planes": P, "groups": groups, "calls_per_group": 5, "input_sets": sets,
           "forward_backward": alternated({"kernels": fused, "kernels_pair_form": fused_pair, "float32_tensor_expressions": expressions}, groups)}
    fb = res["forward_backward"]
    res["tensor_expressions_over_kernels"] = fb["float32_tensor_expressions"]["us"] / fb["kernels"]["us"]
    counts = library_launches(lambda: fused(0))
    res["launches"] = {"kernels_library": counts, "kernels_library_total": sum(counts.values()),
                       "kernels_device_total": device_kernels(lambda: fused(0)),
                       "float32_tensor_expressions_device_total": device_kernels(lambda: expressions(0))}
    res["workspace_bytes"] = int(_lib.lib().gsvc_msssim_loss_workspace_bytes(P, H, W))
    return res


def bench_accuracy(dev):
    from gsvc_amd.loss_utils import ms_ssim_l1
    from tests import _msssim_loss_ref as mr
    out = []
    for sigma in mr.SIGMAS:
        x, y = (t.float().to(dev) for t in mr.pictures(H, W, P, sigma))
        xd, yd = x.double(), y.double()
        ms64 = float(mr.ms_ssim_l1(xd, yd)[0])
        g64 = mr.grad_autograd(xd, yd, G_MS, G_L1)
        scale = float(g64.abs().max())
        ms32 = float(mr.ms_ssim_l1(x, y)[0])
        g32 = mr.grad_autograd(x, y, G_MS, G_L1)
        a = x.clone().requires_grad_(True)
        ms, l1 = ms_ssim_l1(a, y)
        (G_MS * ms + G_L1 * l1).backward()
        out.append({"H": H, "W": W, "planes": P, "sigma": sigma, "ms_ssim_float64": ms64,
                    "value_error_kernels": abs(float(ms.double()) - ms64), "value_error_float32_tensor_expressions": abs(ms32 - ms64),
                    "gradient_error_kernels": float((a.grad.double() - g64).abs().max()) / scale,
                    "gradient_error_float32_autograd": float((g32.double() - g64).abs().max()) / scale})
        del g64, g32, xd, yd
        torch.cuda.empty_cache()
    return out


def bench_step(frames, anchors, groups, dev, distortions):
    from gsvc_amd.arguments import cfg_20240919
    from gsvc_amd.fit_setup import configure_fit, new_fit
    from gsvc_amd.frame import SyntheticFrameCube
    fits = {}
    for d in distortions:
        cube = SyntheticFrameCube(H, W, frames, seed=1234, device=dev).materialize()
        mp_, opt, pipe = cfg_20240919()
        opt.optical_lambda = 0.0
        configure_fit(mp_, opt, cube, 40_000, 0.004, min(16.0, float(frames)), None)      # (the reference's schedule: these steps are full precision)
        if d != "ssim":
            opt.distortion = d
        pc, trainer = new_fit(cube, mp_, opt, pipe, anchors, dev)
        fits[d] = [trainer, 0]

    def run(d, steps):
        trainer, it = fits[d]
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            it += 1
            trainer.step(it)
        b.record()
        b.synchronize()
        fits[d][1] = it
        return a.elapsed_time(b) * 1e-3 / steps
    for d in fits:
        run(d, 30)
    times = {d: [] for d in fits}
    for _ in range(groups):          # alternated
        for d in fits:
            times[d].append(run(d, 10))
    launches = {}
    for d in fits:
        fits[d][1] += 1
        trainer, it = fits[d]
        launches[d] = sum(library_launches(lambda: trainer.step(it)).values())
    for trainer, _ in fits.values():
        trainer.close()
    med = {d: statistics.median(v) for d, v in times.items()}
    res = {"H": H, "W": W, "frames": frames, "anchors_init": anchors, "groups": groups, "steps_per_group": 10,
           "ms_per_step": {d: 1e3 * med[d] for d in med}, "ms_per_step_min_max": {d: [1e3 * min(v), 1e3 * max(v)] for d, v in times.items()},
           "library_launches_per_step": launches}
    if "ms_ssim" in med:
        res["ms_ssim_over_ssim"] = med["ms_ssim"] / med["ssim"]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--step-frames", type=int, default=16, help="frames of the 1080p synthetic video of the step measurement")
    ap.add_argument("--anchors", type=int, default=100_000)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--ssim-step-only", action="store_true", help="only the step with the single-scale SSIM: the baseline on a parent checkout")
    ap.add_argument("--baseline", default=None, metavar="JSON", help="the output of --ssim-step-only on the parent commit, recorded beside the step")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_msssim_loss.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "bench_msssim_loss", "device": torch.cuda.get_device_name(dev)}
    if args.ssim_step_only:
        res["step"] = bench_step(args.step_frames, args.anchors, args.groups, dev, ("ssim",))
    else:
        res["loss"] = bench_loss(args.groups, dev)
        res["accuracy"] = bench_accuracy(dev)
        if not args.no_step:
            res["step"] = bench_step(args.step_frames, args.anchors, args.groups, dev, ("ssim", "ms_ssim"))
            if args.baseline:
                with open(args.baseline) as f:
                    base = json.loads(f.read().strip().splitlines()[-1])["step"]
                res["step"]["parent_commit_ssim_ms_per_step"] = base["ms_per_step"]["ssim"]
                res["step"]["parent_commit_ssim_ms_per_step_min_max"] = base["ms_per_step_min_max"]["ssim"]
                res["step"]["ssim_over_parent_commit_ssim"] = res["step"]["ms_per_step"]["ssim"] / base["ms_per_step"]["ssim"]
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
