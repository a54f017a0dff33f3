#!/usr/bin/env python3
"""What the temporal prefilter costs, and one pair of fits with and without it (csrc/tfilter.hip, k_tfilter and k_noise_sums;
gsvc_amd/tfilter.py).  One JSON line.

  kernel    a resident 1080 x 1920 clip of 12 frames, yuv420p and yuv420p10le: the synthetic video's codes with white noise.  The 8
            targets that have all four neighbours, their flows estimated once (``neighbour_flows``).  ``temporal_filter`` alternated in
            the same process with
              copy     a device copy of the bytes the kernel moves per target: five frames of codes and four flow fields;
              torch    the same arithmetic as tensor expressions (int64), checked equal to the kernel before anything is timed;
            and ``noise_sums`` alternated with ``metrics.picture_hash`` on the same frames.  Device-event time of groups of 10 calls
            (the tensor expressions: 1), median over >= 20 groups, per frame.  The flows of one call (531 MB) alone exceed the 256 MiB
            Infinity Cache.
  gop       ``denoise_frames`` of a 64-frame 1080p GOP, flows included: host clock around a final synchronise, median of 3.
  fits      (--fits) one pair of deterministic 2 000-step fits of the 64-frame 1080p synthetic clip with white noise of a known sigma
            on its codes: ``tools/fit_synthetic.py --video noisy.y4m`` as it is and with ``--denoise auto``, each in a fresh process with
            GSVC_DETERMINISTIC=1.  Both decoded videos are compared (``metrics.compare_videos``, all 64 frames) with the CLEAN clip and
            with the noisy source.  One fit each, no repeat, no second seed.  The pair is run twice: as above (a video file without
            flow files: the flow-guided loss is off), and with ``--estimate-flow`` (the flow of the frames the fit is given).

    python tools/bench_tfilter.py [--groups 20] [--no-gop] [--fits [--sigma 3.0 --steps 2000]] [--json profiles/tfilter.json]
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
from gsvc_amd import tfilter as TF  # noqa: E402
from gsvc_amd.frames_out import FrameFormat  # noqa: E402

H, W = 1080, 1920


def timed_group(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(launches):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches          # seconds per call


def noisy_clip(T, fmt, sigma, dev, seed=3):
    """(clean, noisy): uint8 [T, frame_bytes] codes of the synthetic video, and the same with white Gaussian noise of ``sigma`` codes (of
    the format's depth) on every sample, rounded and clipped to the code range."""
    from gsvc_amd.frame import SyntheticFrameCube
    cube = SyntheticFrameCube(H, W, T, seed=1234, device=dev)
    rows = []
    for t in range(0, T, 8):
        rows.append(fo.frames_to_u8([cube._image(k) for k in range(t, min(t + 8, T))], fmt).clone())
    clean = torch.cat(rows)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    peak = (1 << fmt.depth) - 1
    codes = clean.to(torch.float32) if fmt.depth == 8 else (clean.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float32)
    codes = torch.clamp(torch.round(codes + sigma * torch.randn(codes.shape, generator=g, device=dev)), 0, peak)
    noisy = codes.to(torch.uint8) if fmt.depth == 8 else codes.to(torch.int32).to(torch.int16).view(torch.uint8)
    return clean, noisy.contiguous()


# ---- the tensor-expression form ----------------------------------------------------------------------------------------------
def _planes(frames, fmt):
    n = frames.shape[0]
    codes = frames.to(torch.int64) if fmt.depth == 8 else frames.view(torch.int16).to(torch.int64) & 0xFFFF
    ch, cw = H // 2, W // 2
    return [codes[:, :H * W].reshape(n, H, W), codes[:, H * W:H * W + ch * cw].reshape(n, ch, cw), codes[:, H * W + ch * cw:].reshape(n, ch, cw)]


def _predict(a, mvx, mvy, unit):
    n, h, w = a.shape
    X = torch.arange(w, device=a.device)[None, None, :]
    Y = torch.arange(h, device=a.device)[None, :, None]
    px, py = torch.clamp(unit * X + mvx, 0, unit * (w - 1)), torch.clamp(unit * Y + mvy, 0, unit * (h - 1))
    x0, y0 = torch.clamp(px // unit, max=w - 2), torch.clamp(py // unit, max=h - 2)
    fx, fy = px - unit * x0, py - unit * y0
    flat = a.reshape(n, -1)
    at = y0 * w + x0
    g = lambda off: torch.gather(flat, 1, (at + off).reshape(n, -1)).reshape(n, h, w)          # noqa: E731
    s = (unit - fx) * (unit - fy) * g(0) + fx * (unit - fy) * g(1) + (unit - fx) * fy * g(w) + fx * fy * g(w + 1)
    return (s + unit * unit // 2) // (unit * unit)


def torch_filter(frames, fmt, flows, q, first, params=None):
    """The filtered targets first .. first + n - 1 (all with four neighbours) of [T, frame_bytes] yuv420p frames, as tensor expressions."""
    p = params or TF.TemporalFilterParams()
    dev, n = frames.device, flows.shape[0]
    lut_b, lut_p = torch.tensor(p.lut_b, dtype=torch.int64, device=dev), torch.tensor(p.lut_p, dtype=torch.int64, device=dev)
    planes = _planes(frames, fmt)
    cur = [pl[first:first + n] for pl in planes]
    num, den = [256 * c for c in cur], [torch.full_like(c, 256) for c in cur]
    hb, wb = -(-H // 8), -(-W // 8)
    for j, d in enumerate(TF.OFFSETS):
        mv = torch.clamp(torch.round(4.0 * flows[:, j]), -32768, 32767).to(torch.int64)          # (round: half to even)
        nb = [pl[first + d:first + d + n] for pl in planes]
        pred_y = _predict(nb[0], mv[:, 0], mv[:, 1], 4)
        sq = torch.nn.functional.pad((cur[0] - pred_y) ** 2, (0, 8 * wb - W, 0, 8 * hb - H))
        sse = sq.reshape(n, hb, 8, wb, 8).sum((2, 4))
        cnt = torch.nn.functional.pad(torch.ones((1, H, W), dtype=torch.int64, device=dev), (0, 8 * wb - W, 0, 8 * hb - H)).reshape(1, hb, 8, wb, 8).sum((2, 4))
        ib = torch.clamp(2048 * sse // (cnt * q[0] * q[0]), max=63).repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W]
        for k in range(3):
            if k == 0:
                pred, ibk = pred_y, ib
            else:
                pred, ibk = _predict(nb[k], mv[:, 0, 0::2, 0::2], mv[:, 1, 0::2, 0::2], 8), ib[:, 0::2, 0::2]
            ip = torch.clamp(128 * (cur[k] - pred).abs() // q[k], max=63)
            w = (p.wt[abs(d) - 1] * lut_b[ibk] * lut_p[ip] + (1 << 15)) >> 16
            num[k] = num[k] + w * pred
            den[k] = den[k] + w
    codes = torch.cat([((a + b // 2) // b).reshape(n, -1) for a, b in zip(num, den)], 1)
    return codes.to(torch.uint8) if fmt.depth == 8 else codes.to(torch.int16).view(torch.uint8)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
def bench_case(depth, groups, dev, sigma8=3.0):
    from gsvc_amd.metrics import picture_hash
    fmt = FrameFormat("yuv420p", depth=depth)
    nb = fo.frame_bytes(H, W, fmt)
    T, first, n = 12, 2, 8
    sigma = sigma8 * (1 << (depth - 8))
    _, clip = noisy_clip(T, fmt, sigma, dev)
    est, q = TF.noise_strength(TF.noise_sums(clip, H, W, fmt), H, W, fmt)
    flows = TF.neighbour_flows(TF.code_lumas(clip, H, W, fmt), first, n)
    out = torch.empty((n, nb), dtype=torch.uint8, device=dev)
    TF.temporal_filter(clip, H, W, fmt, flows, q, out=out, first=first)
    equal = bool(torch.equal(torch_filter(clip, fmt, flows[:2], q, first), out[:2]))
    again = torch.empty_like(out)
    TF.temporal_filter(clip, H, W, fmt, flows, q, out=again, first=first)
    same = bool(torch.equal(again, out))
    moved = n * (5 * nb + 4 * 2 * H * W * 4)              # per call: five frames of codes and four flow fields per target
    src, dst = torch.empty(moved, dtype=torch.uint8, device=dev), torch.empty(moved, dtype=torch.uint8, device=dev)
    src.random_(0, 256)

    def tfilter(k):
        return TF.temporal_filter(clip, H, W, fmt, flows, q, out=out, first=first)

    def copy(k):
        return dst.copy_(src)

    def noise(k):
        return TF.noise_sums(clip, H, W, fmt)

    def phash(k):
        return picture_hash(clip, H, W, fmt)

    def expr(k):
        return torch_filter(clip, fmt, flows[:2], q, first)
    fast, slow = (tfilter, copy, noise, phash), (expr,)
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
    per = {"tfilter": n, "copy": n, "noise": T, "phash": T, "expr": 2}
    res = {"case": f"tfilter_{fmt.name}_1080p", "H": H, "W": W, "clip_frames": T, "targets_per_call": n, "groups": groups, "calls_per_group": 10,
           "frame_bytes": nb, "bytes_moved_per_target": moved // n, "noise_sigma_added": sigma, "noise_sigma_estimated": list(est), "q": list(q),
           "filter_equals_torch": equal, "filter_two_runs_same_bits": same}
    for name, key in (("tfilter", "tfilter"), ("copy", "copy"), ("torch_filter", "expr"), ("noise_sums", "noise"), ("picture_hash", "phash")):
        res[name + "_us_per_frame"] = 1e6 * med[key] / per[key]
        res[name + "_us_per_frame_min_max"] = [1e6 * min(t[key]) / per[key], 1e6 * max(t[key]) / per[key]]
    res.update(tfilter_over_copy=res["tfilter_us_per_frame"] / res["copy_us_per_frame"],
               torch_over_tfilter=res["torch_filter_us_per_frame"] / res["tfilter_us_per_frame"],
               noise_sums_over_picture_hash=res["noise_sums_us_per_frame"] / res["picture_hash_us_per_frame"],
               tfilter_bytes_per_s=(moved / n + nb) / (1e-6 * res["tfilter_us_per_frame"]),
               copy_bytes_per_s=2 * (moved / n) / (1e-6 * res["copy_us_per_frame"]))
    del clip, flows, src, dst, out, again
    torch.cuda.empty_cache()
    return res


def bench_gop(dev, frames=64, repeats=3, sigma=3.0):
    fmt = FrameFormat("yuv420p")
    clean, clip = noisy_clip(frames, fmt, sigma, dev)
    TF.denoise_frames(clip[:8], H, W, fmt)
    torch.cuda.synchronize()
    secs, log, out = [], None, None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, log = TF.denoise_frames(clip, H, W, fmt)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    from gsvc_amd.metrics import plane_sse, psnr_of_sse
    psnr = lambda a: float(psnr_of_sse(plane_sse(a, clean, H, W, fmt)[:, 0].sum(), frames * H * W, 255.0))          # noqa: E731
    return {"frames": frames, "H": H, "W": W, "format": fmt.name, "chunk": 8, "repeats": repeats, "seconds": statistics.median(secs),
            "seconds_min_max": [min(secs), max(secs)], "ms_per_frame": 1e3 * statistics.median(secs) / frames, "noise_sigma_added": sigma,
            "log": log, "psnr_y_noisy_vs_clean": psnr(clip), "psnr_y_filtered_vs_clean": psnr(out)}


# ---- the pair of fits ------------------------------------------------------------------------------------------------------------
def _mean(d):
    """The means over the frames that ``compare_videos`` reports."""
    return {k: d[k] for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_611", "psnr_avg", "msssim_y") if k in d}


def bench_fits(dev, sigma, steps, frames=64, fit_args=()):
    from gsvc_amd.metrics import compare_videos
    fmt = FrameFormat("yuv420p")
    clean, noisy = noisy_clip(frames, fmt, sigma, dev)
    est, _ = TF.noise_strength(TF.noise_sums(noisy, H, W, fmt), H, W, fmt)
    out = {"clip": "SyntheticFrameCube(1080, 1920, 64, seed=1234) as yuv420p codes + white Gaussian noise", "frames": frames, "steps": steps,
           "fit_args": list(fit_args), "noise_sigma_added": sigma, "noise_sigma_estimated": list(est), "fits": {}}
    with tempfile.TemporaryDirectory() as tmp:
        paths = {"clean": os.path.join(tmp, "clean.y4m"), "noisy": os.path.join(tmp, "noisy.y4m")}
        for name, rows in (("clean", clean), ("noisy", noisy)):
            with fo.Y4MWriter(paths[name], W, H, (30, 1), fmt) as sink:
                for row in rows.cpu():
                    sink.write(row)
        del clean, noisy
        torch.cuda.empty_cache()
        out["noisy_vs_clean"] = _mean(compare_videos(paths["noisy"], paths["clean"]))
        for name, extra in (("as_it_is", []), ("denoise_auto", ["--denoise", "auto"])):
            dec, log_path = os.path.join(tmp, name + ".y4m"), os.path.join(tmp, name + ".json")
            cmd = [sys.executable, os.path.join(ROOT, "tools", "fit_synthetic.py"), "--video", paths["noisy"], "--steps", str(steps), "--code-metrics",
                   "--write-decoded", dec, "--json", log_path, "--payload-tol", "1"] + list(fit_args) + extra          # (the tool's own 2 % check of the
            # entropy estimate is not this measurement's subject; the ratio is recorded)
            subprocess.run(cmd, check=True, env=dict(os.environ, GSVC_DETERMINISTIC="1"), stdout=sys.stderr, timeout=900)          # (the fit's own progress lines go to stderr)
            with open(log_path) as f:
                log = json.load(f)
            out["fits"][name] = {"bpp": log["bpp"], "fit_seconds": log["fit_seconds"], "anchors_coded": log["anchors_coded"],
                                 "denoise": log.get("denoise"), "attribute_payload_vs_estimate": log["attribute_payload_vs_estimate"], "vs_clean": _mean(compare_videos(dec, paths["clean"])),
                                 "vs_noisy_source": _mean(compare_videos(dec, paths["noisy"]))}
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-gop", action="store_true")
    ap.add_argument("--fits", action="store_true", help="also run the pair of 1080p fits (two fresh processes, minutes)")
    ap.add_argument("--sigma", type=float, default=3.0, help="the white noise of the pair of fits, in 8-bit codes")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tfilter.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "bench_tfilter", "device": torch.cuda.get_device_name(dev), "kernel": []}
    with torch.no_grad():
        if not args.no_kernel:
            for depth in (8, 10):
                res["kernel"].append(bench_case(depth, max(args.groups, 20), dev))
        if not args.no_gop:
            res["gop"] = bench_gop(dev)
        if args.fits:
            res["fits"] = bench_fits(dev, args.sigma, args.steps)          # (a --video without flow files: optical_lambda = 0)
            res["fits_estimated_flow"] = bench_fits(dev, args.sigma, args.steps, fit_args=("--estimate-flow",))
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
