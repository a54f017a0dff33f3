#!/usr/bin/env python3
"""What the detail map and the point sampler cost (csrc/detail.hip, k_frames_detail and k_detail_sample).  One
JSON line.

  kernel    1080 x 1920 and 2160 x 3840 buffers of n = 8 frames, yuv420p and yuv420p10le, of a synthetic video (``SyntheticFrameCube``
            converted by ``frames_to_u8``, tiled up to 2160p).  ``detail.luma_detail`` at cell 8 and, alternated with it in the same
            process, three yardsticks on the SAME buffers:
              copy    a device copy of the bytes the kernel reads (the luma planes: a strided ``copy_``);
              hash    ``metrics.picture_hash`` (k_picture_hash walks whole frames: 1.5 times the bytes);
              torch   the same map as tensor expressions (clamped shifts, abs, an integer ``avg_pool``-style reshape sum).
            Device-event time of groups of 20 calls (the tensor expressions: 2), median over >= 30 groups, per frame; algorithmic bytes =
            the luma plane once (the neighbour's plane is another frame's own plane: in a call of n frames each plane is needed once
            from HBM, the second read may come from the cache; the figure is conservative), their rate and its share of the 8 TB/s HBM
            peak (a KERNEL's share of peak).  The inputs rotate through enough sets to exceed the 256 MiB Infinity Cache.
  sampler   ``detail.sample_points`` at N = 100 000 on the cell-8 map of 64 frames of 1080p (the cumsum, the two allocations and the
            launch), and the launch alone on a prepared prefix sum.

    python tools/bench_detail.py [--groups 30] [--json profiles/detail_init.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsvc_amd import _lib, detail, metrics  # noqa: E402
from gsvc_amd import frames_out as fo  # noqa: E402
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


def make_sets(H, W, fmt, n, sets, dev):
    """``sets`` buffers [n, frame_bytes]: a 1080p synthetic video, tiled 2 x 2 for 2160p; each set starts at another frame."""
    from gsvc_amd.frame import SyntheticFrameCube
    bh, bw = (H, W) if H <= 1080 else (H // 2, W // 2)
    cube = SyntheticFrameCube(bh, bw, n + sets, seed=3, device=dev)
    imgs = [cube._image(t) for t in range(n + sets)]
    if (bh, bw) != (H, W):
        imgs = [im.repeat(1, 2, 2) for im in imgs]
    return [fo.frames_to_u8(imgs[k:k + n], fmt).contiguous() for k in range(sets)]


def torch_detail(frames_u8, H, W, fmt, cell):
    """[n, frame_bytes] -> int64 [n, Hc, Wc]: the map as tensor expressions."""
    n = frames_u8.shape[0]
    if fmt.depth == 8:
        Y = frames_u8[:, :H * W].to(torch.int32)
    else:
        Y = frames_u8[:, :2 * H * W].view(torch.int16).to(torch.int32) & 0xFFFF
    Y = Y.reshape(n, H, W)
    right, left = torch.cat([Y[:, :, 1:], Y[:, :, -1:]], 2), torch.cat([Y[:, :, :1], Y[:, :, :-1]], 2)
    down, up = torch.cat([Y[:, 1:], Y[:, -1:]], 1), torch.cat([Y[:, :1], Y[:, :-1]], 1)
    e = (right - left).abs() + (down - up).abs()
    if n > 1:
        nb = torch.cat([Y[1:], Y[-2:-1]], 0)
        e = e + 2 * (nb - Y).abs()
    Hc, Wc = detail.map_shape(H, W, cell)
    e = torch.nn.functional.pad(e, (0, Wc * cell - W, 0, Hc * cell - H))
    return e.reshape(n, Hc, cell, Wc, cell).to(torch.int64).sum(dim=(2, 4))


def bench_case(H, W, depth, n, groups, dev):
    fmt = FrameFormat("yuv420p", depth=depth)
    nb = fo.frame_bytes(H, W, fmt)
    luma = H * W * (2 if depth > 8 else 1)
    sets = max(2, -(-CACHE // (n * nb)))
    bufs = make_sets(H, W, fmt, n, sets, dev)
    dst = torch.empty((n, luma), dtype=torch.uint8, device=dev)

    def det(k):
        return detail.luma_detail(bufs[k % sets], H, W, fmt, 8)

    def copy(k):
        return dst.copy_(bufs[k % sets][:, :luma])

    def hash_(k):
        return metrics.picture_hash(bufs[k % sets], H, W, fmt)

    def expr(k):
        return torch_detail(bufs[k % sets], H, W, fmt, 8)
    first = det(0)
    same = bool(torch.equal(first, det(0)))
    equal = bool(torch.equal(expr(0), first.view(torch.int32).to(torch.int64) & 0xFFFFFFFF))
    for _ in range(3):
        for fn in (det, copy, hash_):
            timed_group(fn, 20)
        timed_group(expr, 2)
    td, tc, th, te = [], [], [], []
    for _ in range(groups):          # alternated
        td.append(timed_group(det, 20))
        tc.append(timed_group(copy, 20))
        th.append(timed_group(hash_, 20))
        te.append(timed_group(expr, 2))
    d, c, h, e = (statistics.median(t) for t in (td, tc, th, te))
    res = {"case": f"detail_{fmt.name}_{H}p", "H": H, "W": W, "cell": 8, "frames_per_call": n, "groups": groups, "calls_per_group": 20,
           "input_sets": sets, "luma_bytes_per_frame": luma, "frame_bytes": nb,
           "detail_us_per_frame": 1e6 * d / n, "detail_us_per_frame_min_max": [1e6 * min(td) / n, 1e6 * max(td) / n],
           "copy_us_per_frame": 1e6 * c / n, "copy_us_per_frame_min_max": [1e6 * min(tc) / n, 1e6 * max(tc) / n],
           "hash_us_per_frame": 1e6 * h / n, "hash_us_per_frame_min_max": [1e6 * min(th) / n, 1e6 * max(th) / n],
           "torch_us_per_frame": 1e6 * e / n, "torch_us_per_frame_min_max": [1e6 * min(te) / n, 1e6 * max(te) / n],
           "detail_over_copy": d / c, "detail_over_hash": d / h, "torch_over_detail": e / d,
           "detail_luma_bytes_per_s": luma * n / d, "detail_share_of_hbm_peak_8TBps": luma * n / d / HBM_PEAK,
           "copy_read_share_of_hbm_peak_8TBps": luma * n / c / HBM_PEAK, "two_runs_same_bits": same, "torch_equals_kernel": equal}
    del bufs, dst
    torch.cuda.empty_cache()
    return res


def bench_sampler(groups, dev):
    from gsvc_amd.frame import SyntheticFrameCube
    H, W, T, N = 1080, 1920, 64, 100_000
    fmt = FrameFormat("yuv420p")
    cube = SyntheticFrameCube(H, W, T, seed=3, device=dev)
    dmap = torch.cat([detail.luma_detail(fo.frames_to_u8([cube._image(t) for t in range(s, min(s + 16, T))], fmt), H, W, fmt, 8)
                      for s in range(0, T, 16)])          # (per-chunk maps: the timing does not need the overlap)
    cdf = torch.cumsum((dmap.view(torch.int32).to(torch.int64) & 0xFFFFFFFF).reshape(-1), 0)
    points = torch.empty((N, 3), dtype=torch.float32, device=dev)
    cell_of = torch.empty((N,), dtype=torch.int32, device=dev)
    L, stream = _lib.lib(), _lib.current_stream(dev)

    def whole(k):
        return detail.sample_points(dmap, H, W, 8, N, 0.25, k)

    def launch(k):
        _lib.check(L.gsvc_detail_sample(cdf.data_ptr(), int(cdf.shape[0]), T, H, W, 8, N, k, 1 << 22, points.data_ptr(), cell_of.data_ptr(), stream),
                   "gsvc_detail_sample")
    for _ in range(3):
        timed_group(whole, 20)
        timed_group(launch, 20)
    tw, tl = [], []
    for _ in range(groups):
        tw.append(timed_group(whole, 20))
        tl.append(timed_group(launch, 20))
    return {"case": "sampler_1080p_64_frames", "N": N, "cells": int(cdf.shape[0]), "mix": 0.25, "groups": groups, "calls_per_group": 20,
            "sample_points_us": 1e6 * statistics.median(tw), "sample_points_us_min_max": [1e6 * min(tw), 1e6 * max(tw)],
            "launch_alone_us": 1e6 * statistics.median(tl), "launch_alone_us_min_max": [1e6 * min(tl), 1e6 * max(tl)]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=30)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_detail.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "bench_detail", "device": torch.cuda.get_device_name(dev), "kernel": []}
    with torch.no_grad():
        for H, W in ((1080, 1920), (2160, 3840)):
            for depth in (8, 10):
                res["kernel"].append(bench_case(H, W, depth, 8, max(args.groups, 30), dev))
        res["sampler"] = bench_sampler(max(args.groups, 30), dev)
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
