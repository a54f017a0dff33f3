#!/usr/bin/env python3
"""What the encoder's 8-bit input stage costs (csrc/frames_in.hip, gsvc_amd/frames_in.py).  One process, one JSON line.

  kernel   per size (1080 x 1920, 2160 x 3840), layout (rgb24, yuv444p, yuv420p) and — 4:2:0 — chroma mode, n = 8 frames per launch:
           device-event time of groups of 20 launches, median over >= 30 groups, per frame; algorithmic bytes per frame
           frame_bytes + 12 H W from the shapes; achieved bytes/s and its share of the 8 TB/s HBM peak (a KERNEL's share of peak, not
           an end-to-end rate).  Inputs and outputs rotate through enough sets to exceed the 256 MiB Infinity Cache, so the traffic
           is HBM's.
  torch    the same conversion written as the tensor expressions a user would write without the kernel (float(), the matrix as
           broadcast arithmetic, F.interpolate, clamp), same inputs, groups alternated with the kernel's in the same process;
           ratio = torch / kernel.  ``max_abs_difference_kernel_vs_torch`` says that the two compute the same thing.

    python tools/bench_frames_in.py [--groups 30] [--sizes 1080x1920,2160x3840] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsvc_amd import frames_in as fi  # noqa: E402
from gsvc_amd import frames_out as fo  # noqa: E402
from gsvc_amd.frames_out import FrameFormat  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s (MI355X)
MATRIX = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114)}


def torch_convert(frames, H, W, fmt: FrameFormat, chroma):
    """The conversion as tensor expressions: uint8 [n, frame_bytes] -> float32 [n, 3, H, W]."""
    n = frames.shape[0]
    if fmt.layout == "rgb24":
        return frames.view(n, H, W, 3).permute(0, 3, 1, 2).float().div(255.0).contiguous()
    ch, cw = (H // 2, W // 2) if fmt.layout == "yuv420p" else (H, W)
    y = frames[:, :H * W].view(n, 1, H, W).float()
    u = frames[:, H * W:H * W + ch * cw].view(n, 1, ch, cw).float()
    v = frames[:, H * W + ch * cw:].view(n, 1, ch, cw).float()
    if fmt.layout == "yuv420p":
        kw = dict(mode="bilinear", align_corners=False) if chroma == "bilinear" else dict(mode="nearest")
        u = torch.nn.functional.interpolate(u, scale_factor=2, **kw)
        v = torch.nn.functional.interpolate(v, scale_factor=2, **kw)
    Kr, Kb = MATRIX[fmt.matrix]
    Kg = 1.0 - Kr - Kb
    yo, yd, cd = (16.0, 219.0, 224.0) if fmt.range == "limited" else (0.0, 255.0, 255.0)
    Y, Cb, Cr = (y - yo) / yd, (u - 128.0) / cd, (v - 128.0) / cd
    R = Y + 2.0 * (1.0 - Kr) * Cr
    B = Y + 2.0 * (1.0 - Kb) * Cb
    G = Y - (2.0 * Kr * (1.0 - Kr) / Kg) * Cr - (2.0 * Kb * (1.0 - Kb) / Kg) * Cb
    return torch.cat([R, G, B], 1).clamp(0.0, 1.0)


def timed_group(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(launches):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches          # seconds per launch


def bench_kernel(H, W, layout, chroma, n, groups, dev):
    fmt = FrameFormat(layout)
    nbytes = fo.frame_bytes(H, W, fmt)
    sets = max(2, -(-(300 << 20) // (n * nbytes)))          # input sets: together more than the 256 MiB last-level cache
    out_sets = max(2, -(-(300 << 20) // (n * 12 * H * W)))
    g = torch.Generator(device=dev).manual_seed(H + len(layout))
    inputs = [torch.randint(0, 256, (n, nbytes), dtype=torch.uint8, device=dev, generator=g) for _ in range(sets)]
    outs = [torch.empty((n, 3, H, W), dtype=torch.float32, device=dev) for _ in range(out_sets)]
    diff = float((fi.frames_from_u8(inputs[0], H, W, fmt, chroma) - torch_convert(inputs[0], H, W, fmt, chroma)).abs().max())

    def kernel(k):
        fi.frames_from_u8(inputs[k % sets], H, W, fmt, chroma, out=outs[k % out_sets])

    def expr(k):
        torch_convert(inputs[k % sets], H, W, fmt, chroma)

    for _ in range(3):
        timed_group(kernel, 20)
        timed_group(expr, 4)
    tk, tt = [], []
    for _ in range(groups):          # alternated
        tk.append(timed_group(kernel, 20))
        tt.append(timed_group(expr, 4))
    k_med, t_med = statistics.median(tk), statistics.median(tt)
    alg = nbytes + 12 * H * W
    return {"H": H, "W": W, "layout": layout, "chroma": chroma if layout == "yuv420p" else None, "n": n, "frame_bytes": nbytes,
            "input_sets": sets, "output_sets": out_sets, "groups": groups, "launches_per_group": 20,
            "kernel_us_per_frame": 1e6 * k_med / n, "kernel_us_per_frame_min_max": [1e6 * min(tk) / n, 1e6 * max(tk) / n],
            "algorithmic_bytes_per_frame": alg, "kernel_bytes_per_s": alg * n / k_med, "kernel_share_of_hbm_peak_8TBps": alg * n / k_med / HBM_PEAK,
            "torch_expressions_us_per_frame": 1e6 * t_med / n, "torch_over_kernel": t_med / k_med, "max_abs_difference_kernel_vs_torch": diff}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=30)
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames_in.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "bench_frames_in", "device": torch.cuda.get_device_name(dev), "kernel": []}
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        for layout, chroma in (("rgb24", "bilinear"), ("yuv444p", "bilinear"), ("yuv420p", "bilinear"), ("yuv420p", "nearest")):
            with torch.no_grad():
                res["kernel"].append(bench_kernel(H, W, layout, chroma, 8, max(args.groups, 30), dev))
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
