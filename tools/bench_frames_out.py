#!/usr/bin/env python3
"""What the decoder's 8-bit output stage costs (csrc/frames_out.hip, gsvc_amd/frames_out.py).  One process, one JSON line.

  kernel   per size (1080 x 1920, 2160 x 3840) and layout (rgb24, yuv444p, yuv420p), n = 8 images per launch: device-event time of
           groups of 20 launches, median over >= 30 groups, per frame; algorithmic bytes per frame 12 H W + frame_bytes from the
           shapes; achieved bytes/s and its share of the 8 TB/s HBM peak (a KERNEL's share of peak, not an end-to-end rate).  The
           inputs rotate through enough image sets to exceed the 256 MiB Infinity Cache, so the reads come from HBM.
  torch    the same conversion written as the tensor expressions a user would write without the kernel (clamp, matrix, avg_pool2d,
           round, to(uint8), cat), same inputs, groups alternated with the kernel's in the same process; ratio = torch / kernel.
  loop     (unless --no-loop) the decoder loop on the fitted headline model of tools/profile_decoder_loop.py (245 k anchors, 1080p,
           48 frames), frames per second of four loops alternated: render_frames with nothing delivered; render_frames + a
           non-blocking float copy of every frame to pinned host memory; render_frames_u8(yuv420p, to_host=True); the same with
           to_host=False.  End-to-end rates (wall clock around a loop that ends in a device synchronise).

    python tools/bench_frames_out.py [--no-loop] [--groups 30] [--anchors 245000] [--fit-steps 200] [--frames 48] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsvc_amd import frames_out as fo  # noqa: E402
from gsvc_amd.frames_out import FrameFormat  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s (MI355X)
MATRIX = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}


def torch_convert(images, fmt: FrameFormat):
    """The conversion as tensor expressions (what a user writes today): uint8 [n, frame_bytes]."""
    x = torch.stack(images).clamp(0.0, 1.0)
    n = x.shape[0]
    half = 0.5 if fmt.rounding_used == "nearest" else 0.0
    if fmt.layout == "rgb24":
        return x.mul(255.0).add(half).to(torch.uint8).permute(0, 2, 3, 1).contiguous().view(n, -1)
    Kr, Kb = MATRIX[fmt.matrix]
    R, G, B = x[:, 0], x[:, 1], x[:, 2]
    Y = Kr * R + (1.0 - Kr - Kb) * G + Kb * B
    Cb, Cr = (B - Y) / (2.0 * (1.0 - Kb)), (R - Y) / (2.0 * (1.0 - Kr))
    if fmt.layout == "yuv420p":
        Cb = torch.nn.functional.avg_pool2d(Cb.unsqueeze(1), 2).squeeze(1)
        Cr = torch.nn.functional.avg_pool2d(Cr.unsqueeze(1), 2).squeeze(1)
    ys, yo, cs = (219.0, 16.0, 224.0) if fmt.range == "limited" else (255.0, 0.0, 255.0)

    def q(v):
        return v.clamp(0.0, 255.0).add(half).to(torch.uint8).flatten(1)
    return torch.cat([q(yo + ys * Y), q(128.0 + cs * Cb), q(128.0 + cs * Cr)], 1)


def timed_group(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(launches):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches          # seconds per launch


def bench_kernel(H, W, layout, n, groups, dev):
    fmt = FrameFormat(layout)
    nbytes = fo.frame_bytes(H, W, fmt)
    sets = max(2, -(-(300 << 20) // (n * 12 * H * W)))          # image sets: together more than the 256 MiB last-level cache
    g = torch.Generator(device=dev).manual_seed(H + len(layout))
    inputs = [[torch.rand((3, H, W), device=dev, generator=g) * 1.2 - 0.1 for _ in range(n)] for _ in range(sets)]
    out = torch.empty((n, nbytes), dtype=torch.uint8, device=dev)
    same = max(int((fo.frames_to_u8(inputs[0], fmt).int() - torch_convert(inputs[0], fmt).int()).abs().max()), 0)

    def kernel(k):
        fo.frames_to_u8(inputs[k % sets], fmt, out=out)

    def expr(k):
        torch_convert(inputs[k % sets], fmt)

    for _ in range(3):
        timed_group(kernel, 20)
        timed_group(expr, 4)
    tk, tt = [], []
    for _ in range(groups):          # alternated
        tk.append(timed_group(kernel, 20))
        tt.append(timed_group(expr, 4))
    k_med, t_med = statistics.median(tk), statistics.median(tt)
    alg = 12 * H * W + nbytes
    return {"H": H, "W": W, "layout": layout, "n": n, "frame_bytes": nbytes, "input_sets": sets, "groups": groups, "launches_per_group": 20,
            "kernel_us_per_frame": 1e6 * k_med / n, "kernel_us_per_frame_min_max": [1e6 * min(tk) / n, 1e6 * max(tk) / n],
            "algorithmic_bytes_per_frame": alg, "kernel_bytes_per_s": alg * n / k_med, "kernel_share_of_hbm_peak_8TBps": alg * n / k_med / HBM_PEAK,
            "torch_expressions_us_per_frame": 1e6 * t_med / n, "torch_over_kernel": t_med / k_med, "max_byte_difference_kernel_vs_torch": same}


def headline_model(anchors, steps, dev):
    """The fitted headline model of tools/profile_decoder_loop.py: (model, cube, pipe, background)."""
    from gsvc_amd.arguments import cfg_20240919
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.model import GaussianModel
    from gsvc_amd.train import Trainer
    mp_, opt, pipe = cfg_20240919()
    cube = SyntheticFrameCube(1080, 1920, 64, seed=1234, device=dev).materialize()
    mp_.threshold = 8.0 / cube.scale
    opt.full_precision_training_total, opt.quantized_training_total = 0, 0
    opt.entropy_constrained_train_total = 10 ** 9
    opt.start_stat, opt.update_until, opt.pause_densification = 0, 10 ** 9, 0
    torch.manual_seed(0)
    np.random.seed(0)
    pc = GaussianModel(mp_, mp_.anchor_feature_dim, mp_.n_offsets, mp_.voxel_size, mp_.update_depth, mp_.update_init_factor,
                       mp_.update_hierarchy_factor, mp_.use_feat_bank, n_features_per_level=mp_.grid_feature_dim,
                       log2_hashmap_size=mp_.log2, log2_hashmap_size_2D=mp_.log2_2D, device=dev)
    lim = np.array([cube.x_min, cube.y_min, cube.z_min]) * 1.1
    pc.create_from_points(np.random.default_rng(0).uniform(lim, -lim, (anchors, 3)), spatial_lr_scale=1.0)
    pc.update_anchor_bound(cube.x_min, cube.y_min, cube.z_min)
    pc.training_setup(opt)
    tr = Trainer(pc, cube, opt, pipe, mp_, seed=0)
    for it in range(1, steps + 1):
        tr.step(it)
    torch.cuda.synchronize()
    bg = tr.background
    tr.close()
    return pc, cube, pipe, bg


def bench_loop(anchors, steps, n_frames, repeats, dev):
    from gsvc_amd.ortho_gaussian_renderer import render_frames
    pc, cube, pipe, bg = headline_model(anchors, steps, dev)
    frames = [cube.get_dummy_frame(i) for i in range(8, 8 + n_frames)]
    pinned = [torch.empty((3, 1080, 1920), dtype=torch.float32, pin_memory=True) for _ in range(16)]
    fmt = FrameFormat("yuv420p")

    def nothing():
        for _ in render_frames(frames, pc, pipe, bg):
            pass

    def float_copy():
        for k, img in enumerate(render_frames(frames, pc, pipe, bg)):
            pinned[k % 16].copy_(img, non_blocking=True)

    checksum = [0]

    def u8_host():
        s = 0
        for f in fo.render_frames_u8(frames, pc, pipe, bg, fmt=fmt, to_host=True):
            s += int(f[0])          # the frame is in host memory when it is handed out
        checksum[0] = s

    def u8_device():
        for _ in fo.render_frames_u8(frames, pc, pipe, bg, fmt=fmt, to_host=False):
            pass

    loops = (("render_frames_nothing_delivered", nothing), ("render_frames_float_copy_to_pinned", float_copy),
             ("render_frames_u8_yuv420p_to_host", u8_host), ("render_frames_u8_yuv420p_on_device", u8_device))
    for _, fn in loops:
        fn()
        fn()
    torch.cuda.synchronize()
    rates = {name: [] for name, _ in loops}
    issue = {name: [] for name, _ in loops}          # host time until the loop returns, before the final synchronise
    for _ in range(repeats):          # alternated
        for name, fn in loops:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            rates[name].append(n_frames / (time.perf_counter() - t0))
            issue[name].append(1e3 * (t1 - t0))
    out = {"anchors": int(pc._anchor.shape[0]), "fit_steps": steps, "frames": n_frames, "repeats": repeats, "H": 1080, "W": 1920}
    for name, r in rates.items():
        out[name + "_fps"] = statistics.median(r)
        out[name + "_fps_min_max"] = [min(r), max(r)]
        out[name + "_host_ms_before_final_sync"] = statistics.median(issue[name])
    base = out["render_frames_nothing_delivered_fps"]
    out["u8_to_host_over_nothing"] = out["render_frames_u8_yuv420p_to_host_fps"] / base
    out["float_copy_over_nothing"] = out["render_frames_float_copy_to_pinned_fps"] / base
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--groups", type=int, default=30)
    ap.add_argument("--anchors", type=int, default=245_000)
    ap.add_argument("--fit-steps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames_out.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "bench_frames_out", "device": torch.cuda.get_device_name(dev), "kernel": []}
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        for layout in ("rgb24", "yuv444p", "yuv420p"):
            with torch.no_grad():
                res["kernel"].append(bench_kernel(H, W, layout, 8, max(args.groups, 30), dev))
            torch.cuda.empty_cache()
    if not args.no_loop:
        res["decoder_loop"] = bench_loop(args.anchors, args.fit_steps, args.frames, args.repeats, dev)
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
