#!/usr/bin/env python3
"""What the resampler costs (csrc/resample.hip, k_resample; gsvc_amd/resample.py), and one pair of fits at full and
at reduced size.  One JSON line.

  kernel    batches of 8 yuv420p / yuv420p10le frames of the synthetic video, 1080p -> 2160p, 2160p -> 1080p and 1080p -> 480 x 270.
            ``resample_frames`` alternated in the same process with
              copy     a device copy whose traffic is the bytes the kernel reads and writes: (input + output) / 2 bytes copied;
              torch    the same arithmetic as tensor expressions (int64, two frames), checked equal to the kernel at the measured size
                       before anything is timed.
            Device-event time of groups of 10 calls (the tensor expressions: 1), median over >= 20 groups, per frame.
  loop      the decoder loop ``render_frames_u8(to_host=True)`` of the fitted headline model of tools/bench_frames_out.py (1080p) without
            ``out_size`` and with ``out_size`` twice the coded size (2160p frames to the host): frames/s, host clock, alternated.
  fits      (--fits) one pair of deterministic 2 000-step fits of the 64-frame 1080p synthetic clip through tools/gsvc_encode.py, full size
            against ``--coded-size 960x540`` at the same ``--lmbda``, each in a fresh process with GSVC_DETERMINISTIC=1, both decoded to
            source size by tools/gsvc_decode.py and compared with the source (``metrics.compare_videos``).  One fit each: one measurement.

    python tools/bench_resample.py [--groups 20] [--no-loop] [--fits [--steps 2000]] [--json profiles/resample.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gsvc_amd import frames_out as fo  # noqa: E402
from gsvc_amd import resample as R  # noqa: E402
from gsvc_amd.frames_out import FrameFormat  # noqa: E402

CASES = (((1920, 1080), (3840, 2160)), ((3840, 2160), (1920, 1080)), ((1920, 1080), (480, 270)))


def timed_group(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(launches):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches          # seconds per call


def synthetic_frames(H, W, T, fmt, dev, first=0, stop=None):
    """The codes of the frames ``first .. stop - 1`` (default: all) of the ``T``-frame synthetic video."""
    from gsvc_amd.frame import SyntheticFrameCube
    cube = SyntheticFrameCube(H, W, T, seed=1234, device=dev)
    return fo.frames_to_u8([cube._image(k) for k in range(first, T if stop is None else stop)], fmt).clone()


# ---- the tensor-expression form ----------------------------------------------------------------------------------------------
def _axis(a, table, dim, shift, rnd):
    """One pass over ``dim`` of int64 ``a``: sum_k c[:, k] a[clamp(first + k)], then (t + rnd) >> shift."""
    first, coef, nt = table
    size = a.shape[dim]
    first, coef = first.to(torch.int64), coef.to(torch.int64)
    acc = None
    for k in range(nt):
        idx = torch.clamp(first + k, 0, size - 1)
        c = coef[:, k].reshape([-1 if d == dim else 1 for d in range(a.dim())])
        term = a.index_select(dim, idx) * c
        acc = term if acc is None else acc + term
    return (acc + rnd) >> shift


def torch_resample(frames, H, W, fmt, oH, oW):
    n, d = frames.shape[0], fmt.depth
    codes = frames.to(torch.int64) if d == 8 else frames.view(torch.int16).to(torch.int64) & 0xFFFF
    out, at = [], 0
    for (h, w), (oh, ow) in zip(((H, W), (H // 2, W // 2), (H // 2, W // 2)), ((oH, oW), (oH // 2, oW // 2), (oH // 2, oW // 2))):
        a = codes[:, at:at + h * w].reshape(n, h, w)
        at += h * w
        m = _axis(a, R.device_taps(w, ow, frames.device), 2, d - 2, 1 << (d - 3))
        u = _axis(m, R.device_taps(h, oh, frames.device), 1, 30 - d, 1 << (29 - d))
        out.append(torch.clamp(u, 0, (1 << d) - 1).reshape(n, -1))
    codes = torch.cat(out, 1)
    return codes.to(torch.uint8) if d == 8 else codes.to(torch.int16).view(torch.uint8)


def bench_case(size, out_size, depth, groups, dev, n=8):
    (W, H), (oW, oH) = size, out_size
    fmt = FrameFormat("yuv420p", depth=depth)
    ib, ob = fo.frame_bytes(H, W, fmt), fo.frame_bytes(oH, oW, fmt)
    frames = synthetic_frames(H, W, n, fmt, dev)
    out = torch.empty((n, ob), dtype=torch.uint8, device=dev)
    R.resample_frames(frames, H, W, fmt, oH, oW, out=out)
    equal = bool(torch.equal(torch_resample(frames[:2], H, W, fmt, oH, oW), out[:2]))
    again = torch.empty_like(out)
    R.resample_frames(frames, H, W, fmt, oH, oW, out=again)
    same = bool(torch.equal(again, out))
    moved = n * (ib + ob)
    src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    src.random_(0, 256)

    def resample(k):
        return R.resample_frames(frames, H, W, fmt, oH, oW, out=out)

    def copy(k):
        return dst.copy_(src)

    def expr(k):
        return torch_resample(frames[:2], H, W, fmt, oH, oW)
    fast, slow = (resample, copy), (expr,)
    for _ in range(2):
        for fn in fast:
            timed_group(fn, 10)
        for fn in slow:
            timed_group(fn, 1)
    t = {fn.__name__: [] for fn in fast + slow}
    for _ in range(groups):          # alternated
        for fn in fast:
            t[fn.__name__].append(timed_group(fn, 10))
        for fn in slow:
            t[fn.__name__].append(timed_group(fn, 1))
    med = {k: statistics.median(v) for k, v in t.items()}
    per = {"resample": n, "copy": n, "expr": 2}
    res = {"case": f"resample_{fmt.name}_{W}x{H}_to_{oW}x{oH}", "W": W, "H": H, "out_W": oW, "out_H": oH, "frames_per_call": n, "groups": groups,
           "calls_per_group": 10, "frame_bytes_in": ib, "frame_bytes_out": ob, "nt_luma_x_y": [R.filter_taps(W, oW)[2], R.filter_taps(H, oH)[2]],
           "resample_equals_torch": equal, "resample_two_runs_same_bits": same}
    for name, key in (("resample", "resample"), ("copy", "copy"), ("torch_resample", "expr")):
        res[name + "_us_per_frame"] = 1e6 * med[key] / per[key]
        res[name + "_us_per_frame_min_max"] = [1e6 * min(t[key]) / per[key], 1e6 * max(t[key]) / per[key]]
    res.update(resample_over_copy=res["resample_us_per_frame"] / res["copy_us_per_frame"],
               torch_over_resample=res["torch_resample_us_per_frame"] / res["resample_us_per_frame"],
               resample_bytes_per_s=(ib + ob) / (1e-6 * res["resample_us_per_frame"]),
               copy_bytes_per_s=(ib + ob) / (1e-6 * res["copy_us_per_frame"]))
    del frames, out, again, src, dst
    torch.cuda.empty_cache()
    return res


# ---- the decoder loop --------------------------------------------------------------------------------------------------------------
def bench_loop(anchors, steps, n_frames, repeats, dev):
    from bench_frames_out import headline_model
    pc, cube, pipe, bg = headline_model(anchors, steps, dev)
    fmt = FrameFormat("yuv420p")
    frames = [cube.get_dummy_frame(i) for i in range(8, 8 + n_frames)]
    H, W = 1080, 1920          # (the headline model's size)
    twice = (2 * H, 2 * W)

    def run(out_size):
        s = 0
        for f in fo.render_frames_u8(frames, pc, pipe, bg, fmt=fmt, to_host=True, out_size=out_size):
            s += int(f[0])          # the frame is in host memory when it is handed out
        return s
    with torch.no_grad():
        for size in (None, twice, None, twice):
            run(size)
        torch.cuda.synchronize()
        rates = {"coded_size": [], "twice": []}
        for _ in range(repeats):          # alternated
            for name, size in (("coded_size", None), ("twice", twice)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(size)
                torch.cuda.synchronize()
                rates[name].append(n_frames / (time.perf_counter() - t0))
    out = {"anchors": int(pc._anchor.shape[0]), "fit_steps": steps, "frames": n_frames, "repeats": repeats, "H": H, "W": W, "out_H": twice[0],
           "out_W": twice[1], "batch": 8}
    for name, r in rates.items():
        out[f"fps_{name}"] = statistics.median(r)
        out[f"fps_{name}_min_max"] = [min(r), max(r)]
    out["twice_over_coded_size"] = out["fps_twice"] / out["fps_coded_size"]
    return out


# ---- the pair of fits ------------------------------------------------------------------------------------------------------------
def bench_fits(dev, steps, lmbda, frames=64, H=1080, W=1920, coded=(960, 540)):
    from gsvc_amd.metrics import compare_videos
    fmt = FrameFormat("yuv420p")
    keys = ("psnr_y", "psnr_u", "psnr_v", "psnr_611", "psnr_avg", "msssim_y")
    out = {"clip": f"SyntheticFrameCube({H}, {W}, {frames}, seed=1234) as yuv420p codes", "frames": frames, "steps": steps, "lmbda": lmbda,
           "coded_size": list(coded), "fits": {}}
    with tempfile.TemporaryDirectory() as tmp:
        source = os.path.join(tmp, "source.y4m")
        with fo.Y4MWriter(source, W, H, (30, 1), fmt) as sink:
            for t in range(0, frames, 8):
                for row in synthetic_frames(H, W, frames, fmt, dev, t, min(t + 8, frames)).cpu():
                    sink.write(row)
        torch.cuda.empty_cache()
        env = dict(os.environ, GSVC_DETERMINISTIC="1")
        for name, extra in (("full_size", []), ("coded_%dx%d" % coded, ["--coded-size", "%dx%d" % coded])):
            coded_file, dec = os.path.join(tmp, name + ".gsvc"), os.path.join(tmp, name + ".y4m")
            cmd = [sys.executable, os.path.join(ROOT, "tools", "gsvc_encode.py"), source, "-o", coded_file, "--steps", str(steps), "--lmbda", str(lmbda)]
            done = subprocess.run(cmd + extra, check=True, env=env, stdout=subprocess.PIPE, timeout=900)
            log = json.loads([line for line in done.stdout.decode().splitlines() if line.startswith("{")][-1])          # (the tool's one JSON line)
            subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gsvc_decode.py"), coded_file, "-o", dec, "--strict"], check=True, env=env,
                           stdout=sys.stderr, timeout=900)
            cmp = compare_videos(dec, source)
            out["fits"][name] = {"bpp": log["bpp"], "total_bytes": log["total_bytes"], "fit_seconds": log["fit_seconds"], "anchors_coded": log["anchors_coded"],
                                 "W": log["W"], "H": log["H"], "display": log.get("display"), "vs_source": {k: cmp[k] for k in keys if k in cmp}}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--anchors", type=int, default=245_000)
    ap.add_argument("--fit-steps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--fits", action="store_true", help="also run the pair of 1080p fits (fresh processes, minutes)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--lmbda", type=float, default=0.004)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "bench_resample", "device": torch.cuda.get_device_name(dev), "kernel": []}
    with torch.no_grad():
        if not args.no_kernel:
            for size, out_size in CASES:
                for depth in (8, 10):
                    res["kernel"].append(bench_case(size, out_size, depth, max(args.groups, 20), dev))
    if not args.no_loop:          # (outside no_grad: the headline model is fitted first)
        res["loop"] = bench_loop(args.anchors, args.fit_steps, args.frames, args.repeats, dev)
    if args.fits:
        with torch.no_grad():
            res["fits"] = bench_fits(dev, args.steps, args.lmbda)
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
