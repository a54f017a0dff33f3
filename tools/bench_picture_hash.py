#!/usr/bin/env python3
"""What the picture hash costs (csrc/picture_hash.hip, k_picture_hash).  One process, one JSON line.

  kernel   1080 x 1920 yuv420p buffers of n = 8 frames, 8-bit and 10-bit: ``metrics.picture_hash`` of one buffer and, as the yardstick,
           ``metrics.plane_sse`` of the same buffer against a second one (k_frames_sse reads twice the bytes).  Device-event time of
           groups of 20 calls, the two alternated in the same process, median over >= 30 groups, per frame; algorithmic bytes from the
           shapes (hash: frame_bytes, SSE: 2 frame_bytes), the bytes/s they give and that figure's share of the 8 TB/s HBM peak (a
           KERNEL's share of peak).  The inputs rotate through enough sets to exceed the 256 MiB Infinity Cache.
  loop     the decoder's render loop to host memory (``bitstream.hashed_frames``: render_frames_u8, the batch's hash taken on the device
           before the host copy) on the fitted headline model of tools/bench_frames_out.py, frames per second with and without the
           hash, alternated; ``verify_over_plain`` is the ratio of the medians: the cost of verification.

    python tools/bench_picture_hash.py [--groups 30] [--no-loop] [--json profiles/picture_hash.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

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


def bench_kernel(H, W, depth, n, groups, dev):
    fmt = FrameFormat("yuv420p", depth=depth)
    nb = fo.frame_bytes(H, W, fmt)
    sets = max(2, -(-CACHE // (2 * n * nb)))
    g = torch.Generator(device=dev).manual_seed(H + depth)

    def frames():
        if depth == 8:
            return torch.randint(0, 256, (n, nb), dtype=torch.uint8, device=dev, generator=g)
        return torch.randint(0, 2 ** depth, (n, nb // 2), dtype=torch.int32, device=dev, generator=g).to(torch.int16).view(torch.uint8)
    pairs = [(frames(), frames()) for _ in range(sets)]

    def hash_(k):
        return metrics.picture_hash(pairs[k % sets][0], H, W, fmt)

    def sse(k):
        return metrics.plane_sse(*pairs[k % sets], H, W, fmt)
    same = bool(torch.equal(hash_(0), hash_(0)))
    for _ in range(3):
        timed_group(hash_, 20)
        timed_group(sse, 20)
    th, ts = [], []
    for _ in range(groups):          # alternated
        th.append(timed_group(hash_, 20))
        ts.append(timed_group(sse, 20))
    h_med, s_med = statistics.median(th), statistics.median(ts)
    return {"case": f"picture_hash_{fmt.name}", "H": H, "W": W, "frames_per_call": n, "groups": groups, "calls_per_group": 20, "input_sets": sets,
            "hash_us_per_frame": 1e6 * h_med / n, "hash_us_per_frame_min_max": [1e6 * min(th) / n, 1e6 * max(th) / n],
            "sse_us_per_frame": 1e6 * s_med / n, "sse_us_per_frame_min_max": [1e6 * min(ts) / n, 1e6 * max(ts) / n],
            "hash_over_sse": h_med / s_med, "hash_not_slower_beyond_spread": max(th) <= min(ts),
            "hash_bytes_per_frame": nb, "sse_bytes_per_frame": 2 * nb,
            "hash_bytes_per_s": nb * n / h_med, "hash_share_of_hbm_peak_8TBps": nb * n / h_med / HBM_PEAK,
            "sse_bytes_per_s": 2 * nb * n / s_med, "sse_share_of_hbm_peak_8TBps": 2 * nb * n / s_med / HBM_PEAK, "two_runs_same_bits": same}


def bench_loop(anchors, steps, n_frames, repeats, dev):
    from gsvc_amd.bitstream import hashed_frames
    from tools.bench_frames_out import headline_model
    pc, cube, pipe, bg = headline_model(anchors, steps, dev)
    frames = [cube.get_dummy_frame(i) for i in range(8, 8 + n_frames)]
    fmt = FrameFormat("yuv420p")

    def run(verify):
        hashes = [] if verify else None
        s = 0
        for f in hashed_frames(frames, pc, pipe, bg, 1080, 1920, fmt, 8, hashes):
            s += int(f[0])          # the frame is in host memory when it is handed out
        return s

    loops = (("plain", lambda: run(False)), ("verify", lambda: run(True)))
    with torch.no_grad():
        for _, fn in loops:
            fn()
            fn()
        torch.cuda.synchronize()
        rates = {name: [] for name, _ in loops}
        for _ in range(repeats):          # alternated
            for name, fn in loops:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                rates[name].append(n_frames / (time.perf_counter() - t0))
    out = {"anchors": int(pc._anchor.shape[0]), "fit_steps": steps, "frames": n_frames, "repeats": repeats, "H": 1080, "W": 1920, "batch": 8,
           "format": fmt.name}
    for name, r in rates.items():
        out[name + "_fps"] = statistics.median(r)
        out[name + "_fps_min_max"] = [min(r), max(r)]
    out["verify_over_plain"] = out["verify_fps"] / out["plain_fps"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--groups", type=int, default=30)
    ap.add_argument("--anchors", type=int, default=245_000)
    ap.add_argument("--fit-steps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_picture_hash.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "bench_picture_hash", "device": torch.cuda.get_device_name(dev), "kernel": []}
    with torch.no_grad():
        for depth in (8, 10):
            res["kernel"].append(bench_kernel(1080, 1920, depth, 8, max(args.groups, 30), dev))
            torch.cuda.empty_cache()
    if not args.no_loop:
        res["loop"] = bench_loop(args.anchors, args.fit_steps, args.frames, args.repeats, dev)
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
