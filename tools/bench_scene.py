#!/usr/bin/env python3
"""What the frame histograms cost (csrc/scene.hip, k_frames_histogram).  One JSON line.

  kernel    1080 x 1920 yuv420p buffers of n = 8 frames, 8-bit and 10-bit, of three contents: uniform noise (a lane's run of equal bins
            has length 1), a constant picture (every lane on one counter) and a synthetic frame (``SyntheticFrameCube`` converted by
            ``frames_to_u8``).  ``metrics.plane_histograms`` and, as the yardstick, ``metrics.picture_hash`` of the SAME buffer
            (k_picture_hash reads the same bytes; section 8g puts it at 0.16 of the HBM peak, bound by its integer arithmetic).
            Device-event time of groups of 20 calls, the two alternated in the same process, median over >= 30 groups, per frame;
            algorithmic bytes from the shapes (frame_bytes), the bytes/s they give and that figure's share of the 8 TB/s HBM peak (a
            KERNEL's share of peak).  The inputs rotate through enough sets to exceed the 256 MiB Infinity Cache.
  torch     the same histograms as tensor expressions: per frame and plane one ``torch.bincount`` of the binned codes.
  variants  ``--variant NAME=LIBRARY``: the same kernel measurement in a child process that loads another build of the library
            (``GSVC_LIB_PATH``), e.g. one built with -DGSVC_HIST_UNITS_PER_LANE=4 (a workgroup walks what k_picture_hash's does) or
            -DGSVC_HIST_NO_RUNS (one LDS atomic per sample): what each of the kernel's two decisions is worth.  The hash kernel is the
            same code in every build: ``hist_over_hash`` compares across processes.

    python tools/bench_scene.py [--groups 30] [--variant units4=/path/libgsvc_hip.so ...] [--json profiles/scene.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsvc_amd import frames_out as fo  # noqa: E402
from gsvc_amd import metrics  # noqa: E402
from gsvc_amd.frames_out import FrameFormat  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s (MI355X)
CACHE = 300 << 20          # rotate through more than the 256 MiB last-level cache
CONTENTS = ("noise", "constant", "synthetic")


def timed_group(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(launches):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches          # seconds per call


def make_sets(content, H, W, fmt, n, sets, dev):
    nb = fo.frame_bytes(H, W, fmt)
    g = torch.Generator(device=dev).manual_seed(H + fmt.depth)
    if content == "synthetic":
        from gsvc_amd.frame import SyntheticFrameCube
        cube = SyntheticFrameCube(H, W, n, seed=3, device=dev)
        one = fo.frames_to_u8([cube._image(t) for t in range(n)], fmt).contiguous()
        return [one.clone() for _ in range(sets)]
    out = []
    for k in range(sets):
        if content == "constant":
            code = (100 + k) << (fmt.depth - 8)
            a = torch.full((n, nb // (2 if fmt.depth > 8 else 1)), code, dtype=torch.int32, device=dev)
        else:
            a = torch.randint(0, 2 ** fmt.depth, (n, nb // (2 if fmt.depth > 8 else 1)), dtype=torch.int32, device=dev, generator=g)
        out.append(a.to(torch.uint8) if fmt.depth == 8 else a.to(torch.int16).view(torch.uint8))
    return out


def torch_histograms(frames_u8, H, W, fmt):
    """[n, frame_bytes] -> int64 [n, 3, 256] with torch.bincount per frame and plane."""
    n = frames_u8.shape[0]
    codes = frames_u8 if fmt.depth == 8 else (frames_u8.view(torch.int16).to(torch.int32) & 0xFFFF)
    bins = (codes.to(torch.int32) >> (fmt.depth - 8)).clamp_(max=255)
    px = H * W
    edges = (0, px, px + px // 4, px + px // 2)
    out = torch.empty((n, 3, 256), dtype=torch.int64, device=frames_u8.device)
    for f in range(n):
        for p in range(3):
            out[f, p] = torch.bincount(bins[f, edges[p]:edges[p + 1]], minlength=256)
    return out


def bench_case(content, H, W, depth, n, groups, dev, with_torch):
    fmt = FrameFormat("yuv420p", depth=depth)
    nb = fo.frame_bytes(H, W, fmt)
    sets = max(2, -(-CACHE // (n * nb)))
    bufs = make_sets(content, H, W, fmt, n, sets, dev)

    def hist(k):
        return metrics.plane_histograms(bufs[k % sets], H, W, fmt)

    def hash_(k):
        return metrics.picture_hash(bufs[k % sets], H, W, fmt)
    first = hist(0)
    same = bool(torch.equal(first, hist(0)))
    sums_ok = first.sum(dim=2).tolist() == [list(metrics.plane_samples(H, W, fmt))] * n
    for _ in range(3):
        timed_group(hist, 20)
        timed_group(hash_, 20)
    th, tk = [], []
    for _ in range(groups):          # alternated
        th.append(timed_group(hist, 20))
        tk.append(timed_group(hash_, 20))
    h_med, k_med = statistics.median(th), statistics.median(tk)
    res = {"case": f"{content}_{fmt.name}", "content": content, "H": H, "W": W, "frames_per_call": n, "groups": groups, "calls_per_group": 20,
           "input_sets": sets, "bytes_per_frame": nb,
           "hist_us_per_frame": 1e6 * h_med / n, "hist_us_per_frame_min_max": [1e6 * min(th) / n, 1e6 * max(th) / n],
           "hash_us_per_frame": 1e6 * k_med / n, "hash_us_per_frame_min_max": [1e6 * min(tk) / n, 1e6 * max(tk) / n],
           "hist_over_hash": h_med / k_med, "hist_bytes_per_s": nb * n / h_med, "hist_share_of_hbm_peak_8TBps": nb * n / h_med / HBM_PEAK,
           "hash_share_of_hbm_peak_8TBps": nb * n / k_med / HBM_PEAK, "two_runs_same_bits": same, "bins_sum_to_plane_samples": sums_ok}
    if with_torch:
        res["torch_equals_kernel"] = bool(torch.equal(torch_histograms(bufs[0], H, W, fmt), first.to(torch.int64)))
        for _ in range(2):
            timed_group(lambda k: torch_histograms(bufs[k % sets], H, W, fmt), 2)
        tt = [timed_group(lambda k: torch_histograms(bufs[k % sets], H, W, fmt), 2) for _ in range(max(groups // 3, 10))]
        res["torch_bincount_us_per_frame"] = 1e6 * statistics.median(tt) / n
        res["torch_over_hist"] = statistics.median(tt) / h_med
    del bufs
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=30)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--variant", action="append", default=[], metavar="NAME=LIBRARY", help="measure another build of the library in a child process")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_scene.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "bench_scene", "device": torch.cuda.get_device_name(dev), "library": os.environ.get("GSVC_LIB_PATH") or "in-tree", "kernel": []}
    with torch.no_grad():
        for depth in (8, 10):
            for content in CONTENTS:
                res["kernel"].append(bench_case(content, 1080, 1920, depth, 8, max(args.groups, 30), dev, not args.no_torch))
    if args.variant:
        res["variants"] = {}
    for item in args.variant:
        name, _, path = item.partition("=")
        if not path or not os.path.exists(path):
            raise SystemExit(f"--variant is NAME=LIBRARY (got {item!r})")
        env = dict(os.environ, GSVC_LIB_PATH=os.path.abspath(path))
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--groups", str(args.groups), "--no-torch"], env=env, capture_output=True,
                             text=True, timeout=900)
        if run.returncode != 0:
            raise SystemExit(f"variant {name}: exit {run.returncode}\n{run.stderr[-2000:]}")
        res["variants"][name] = json.loads(run.stdout.strip().splitlines()[-1])["kernel"]
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
