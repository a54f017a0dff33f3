#!/usr/bin/env python3
"""What the metric kernels cost (csrc/metrics.hip: k_frames_sse, k_msssim_scale / _pool / _finalize) beside the same metrics written
as tensor expressions.  One process, one JSON line.

  cases    per size (1080 x 1920, 2160 x 3840):
             sse      plane SSE of two yuv420p buffers of n = 8 frames, 8-bit and 10-bit        (metrics.plane_sse)
             msssim   MS-SSIM of one float32 picture pair with three channels, P = 3             (metrics.ms_ssim_fused)
                      and of the luma planes of one 10-bit yuv420p frame pair read in place, P = 1 (gsvc_msssim on the codes)
  kernel   device-event time of groups of 20 calls, median over >= 30 groups, per frame; algorithmic bytes from the shapes — SSE:
           2 frame_bytes; MS-SSIM: both pictures read at scale 0 and 2 H W P floats written pooled, then (8 H W P read + 2 H W P
           written) / 4 times 4 / 3 over the scales below (for float input: 10 H W P times 4 / 3) — the bytes/s they give and that
           figure's share of the 8 TB/s HBM peak (a KERNEL's share of peak, not a roof: MS-SSIM is arithmetic, not traffic).  The
           inputs rotate through enough sets to exceed the 256 MiB Infinity Cache.
  torch    the same metric as tensor expressions, same inputs, groups of 4 calls alternated with the kernel's in the same process:
           ``metrics.ms_ssim`` as it stands (for codes: after the conversion to float a user would write), and
           ``((a.int() - b.int()) ** 2).sum()`` per plane.  ``torch_over_kernel`` = the ratio of the medians; ``faster_beyond_spread`` =
           the slowest kernel group is faster than the fastest torch group; ``max_difference`` says that the two compute the same.

    python tools/bench_metrics.py [--groups 30] [--sizes 1080x1920,2160x3840] [--json profiles/metrics.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsvc_amd import frames_out as fo  # noqa: E402
from gsvc_amd import metrics  # noqa: E402
from gsvc_amd.frames_out import FrameFormat  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s (MI355X)
CACHE = 300 << 20          # rotate through more than the 256 MiB last-level cache


def timed_group(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(launches):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches          # seconds per call


def _measure(kernel, expr, groups):
    for _ in range(3):
        timed_group(kernel, 20)
        timed_group(expr, 4)
    tk, tt = [], []
    for _ in range(groups):          # alternated
        tk.append(timed_group(kernel, 20))
        tt.append(timed_group(expr, 4))
    return tk, tt


def _row(case, H, W, n, alg, groups, tk, tt, extra):
    k_med, t_med = statistics.median(tk), statistics.median(tt)
    row = {"case": case, "H": H, "W": W, "frames_per_call": n, "groups": groups, "calls_per_group": [20, 4],
           "kernel_us_per_frame": 1e6 * k_med / n, "kernel_us_per_frame_min_max": [1e6 * min(tk) / n, 1e6 * max(tk) / n],
           "torch_expressions_us_per_frame": 1e6 * t_med / n, "torch_expressions_us_per_frame_min_max": [1e6 * min(tt) / n, 1e6 * max(tt) / n],
           "torch_over_kernel": t_med / k_med, "faster_beyond_spread": max(tk) < min(tt),
           "algorithmic_bytes_per_frame": alg, "kernel_bytes_per_s": alg * n / k_med, "kernel_share_of_hbm_peak_8TBps": alg * n / k_med / HBM_PEAK}
    row.update(extra)
    return row


def _codes(frames, fmt):
    """uint8 [n, frame_bytes] -> int32 codes [n, samples]."""
    return frames.int() if fmt.depth == 8 else frames.view(torch.int16).int() & 0xFFFF


def torch_sse(a, b, H, W, fmt):
    """((a.int() - b.int()) ** 2).sum() per plane -> int64 [n, 3]."""
    ca, cb = _codes(a, fmt), _codes(b, fmt)
    px = H * W
    bounds = (0, px, px + px // 4, px + px // 2)
    return torch.stack([((ca[:, lo:hi] - cb[:, lo:hi]) ** 2).sum(1) for lo, hi in zip(bounds[:-1], bounds[1:])], 1)


def bench_sse(H, W, depth, n, groups, dev):
    fmt = FrameFormat("yuv420p", depth=depth)
    nb = fo.frame_bytes(H, W, fmt)
    sets = max(2, -(-CACHE // (2 * n * nb)))
    g = torch.Generator(device=dev).manual_seed(H + depth)

    def frames():
        if depth == 8:
            return torch.randint(0, 256, (n, nb), dtype=torch.uint8, device=dev, generator=g)
        return torch.randint(0, 2 ** depth, (n, nb // 2), dtype=torch.int32, device=dev, generator=g).to(torch.int16).view(torch.uint8)
    pairs = [(frames(), frames()) for _ in range(sets)]
    diff = int((metrics.plane_sse(*pairs[0], H, W, fmt) - torch_sse(*pairs[0], H, W, fmt)).abs().max())
    tk, tt = _measure(lambda k: metrics.plane_sse(*pairs[k % sets], H, W, fmt), lambda k: torch_sse(*pairs[k % sets], H, W, fmt), groups)
    return _row(f"sse_{fmt.name}", H, W, n, 2 * nb, groups, tk, tt, {"input_sets": sets, "max_difference": diff})


def _msssim_bytes(H, W, P, bytes_per_sample):
    return 2 * bytes_per_sample * H * W * P + 2 * H * W * P + 10 * H * W * P // 3


def bench_msssim_float(H, W, groups, dev):
    P = 3
    sets = max(2, -(-CACHE // (2 * P * H * W * 4)))
    g = torch.Generator(device=dev).manual_seed(H)
    pairs = []
    for _ in range(sets):
        x = torch.rand((1, P, H, W), device=dev, generator=g)
        pairs.append((x, (x + 0.03 * torch.randn((1, P, H, W), device=dev, generator=g)).clamp(0, 1)))
    diff = abs(float(metrics.ms_ssim_fused(*pairs[0])) - float(metrics.ms_ssim(*pairs[0])))
    tk, tt = _measure(lambda k: metrics.ms_ssim_fused(*pairs[k % sets]), lambda k: metrics.ms_ssim(*pairs[k % sets]), groups)
    return _row("msssim_float32_P3", H, W, 1, _msssim_bytes(H, W, P, 4), groups, tk, tt, {"P": P, "input_sets": sets, "max_difference": diff})


def bench_msssim_codes(H, W, groups, dev):
    fmt = FrameFormat("yuv420p", depth=10)
    nb, peak = fo.frame_bytes(H, W, fmt), 1023.0
    sets = max(2, -(-CACHE // (2 * 2 * H * W)))          # (the luma planes are what is read)
    g = torch.Generator(device=dev).manual_seed(H + 1)
    pairs = []
    for _ in range(sets):
        a = torch.randint(0, 1024, (1, nb // 2), dtype=torch.int32, device=dev, generator=g)
        b = (a + torch.randint(-12, 13, a.shape, dtype=torch.int32, device=dev, generator=g)).clamp(0, 1023)
        pairs.append((a.to(torch.int16).view(torch.uint8), b.to(torch.int16).view(torch.uint8)))

    def kernel(k):
        a, b = pairs[k % sets]
        return metrics._msssim_value(metrics._msssim_terms(a, b, 1, H, W, (W, nb // 2), (W, nb // 2), metrics.SAMPLE_U16, peak))

    def expr(k):
        a, b = pairs[k % sets]
        x = (a.view(torch.int16)[:, :H * W].int() & 0xFFFF).float().div(peak).view(1, 1, H, W)
        y = (b.view(torch.int16)[:, :H * W].int() & 0xFFFF).float().div(peak).view(1, 1, H, W)
        return metrics.ms_ssim(x, y)
    diff = abs(float(kernel(0)) - float(expr(0)))
    tk, tt = _measure(kernel, expr, groups)
    return _row("msssim_yuv420p10le_luma_P1", H, W, 1, _msssim_bytes(H, W, 1, 2), groups, tk, tt, {"P": 1, "input_sets": sets, "max_difference": diff})


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=30)
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "bench_metrics", "device": torch.cuda.get_device_name(dev), "rows": []}
    groups = max(args.groups, 30)
    with torch.no_grad():
        for size in args.sizes.split(","):
            H, W = (int(v) for v in size.split("x"))
            for fn, a in ((bench_sse, (H, W, 8, 8)), (bench_sse, (H, W, 10, 8)), (bench_msssim_float, (H, W)), (bench_msssim_codes, (H, W))):
                res["rows"].append(fn(*a, groups, dev))
                torch.cuda.empty_cache()
    res["every_1080p_case_faster_beyond_spread"] = all(r["faster_beyond_spread"] for r in res["rows"] if r["H"] == 1080)
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
