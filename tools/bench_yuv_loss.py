#!/usr/bin/env python3
"""What fitting in the delivered domain costs (csrc/yuv_loss.hip, gsvc_amd/yuv_loss.py).  One JSON line.

  kernels   k_frames_planes (8-bit and 10-bit codes), k_yuv_planes_fwd and k_yuv_planes_bwd (two-view form, with the averaged frame) at
            1080 x 1920 and 2160 x 3840, yuv420p and yuv444p.  Device-event time of groups of 20 calls, each kernel alternated in the
            same process with a device copy that moves the same number of bytes (half read, half written), median over >= 30 groups;
            algorithmic bytes from the shapes, the bytes/s they give and that figure's share of the 8 TB/s HBM peak (a KERNEL's share
            of peak).  Inputs and outputs rotate through enough sets to exceed the 256 MiB Infinity Cache.
  torch     the same transform as tensor expressions (flip, average, three weighted sums, 2x2 mean pooling), forward, and forward +
            backward through autograd, against the kernels' forward and forward + backward.
  step      a fitting step per loss domain, the ``rgb`` and ``yuv420`` legs alternated in one process (two fits alive, groups of 10
            steps ending in a synchronise, median of the groups): on the test clip (64 x 48, 8 frames, 3 000 anchors) and on the 1080p
            synthetic video written as yuv420p and read back (``--step-frames`` frames, 100 000 anchors), full-precision phase.
  launches  the library's kernel launches of one step per domain (``gsvc_profile_enable``) and their difference; the tensor-library
            launches the composed form adds on top (2 x (sums / n) and 2 x stack per ssim_l1 call, one cat per frame's backward) are
            listed from the code, not measured.

    python tools/bench_yuv_loss.py [--groups 30] [--step-frames 16] [--no-step] [--json profiles/yuv_loss.json]
    python tools/bench_yuv_loss.py --write-clip synth.y4m [--height 1080 --width 1920 --frames 64]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsvc_amd import _lib  # noqa: E402
from gsvc_amd import yuv_loss  # noqa: E402
from gsvc_amd.frames_out import LAYOUTS, MATRICES, FrameFormat, frame_bytes  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s (MI355X)
CACHE = 300 << 20          # rotate through more than the 256 MiB last-level cache
SIZES = ((1080, 1920), (2160, 3840))


def timed_group(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(launches):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches          # seconds per call


def alternated(fn, nbytes, groups, dev):
    """Median seconds per call of ``fn`` and of a device copy that moves ``nbytes`` in all, groups of 20 alternated."""
    half = max(16, nbytes // 2)
    sets = max(2, -(-CACHE // nbytes))
    src = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(sets)]
    dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(sets)]

    def copy(k):
        dst[k % sets].copy_(src[k % sets])
    for _ in range(3):
        timed_group(fn, 20)
        timed_group(copy, 20)
    tf, tc = [], []
    for _ in range(groups):
        tf.append(timed_group(fn, 20))
        tc.append(timed_group(copy, 20))
    return statistics.median(tf), statistics.median(tc), [min(tf), max(tf)]


def report(name, H, W, what, nbytes, t, t_copy, span):
    return {"kernel": name, "H": H, "W": W, "case": what, "algorithmic_bytes": nbytes, "us": 1e6 * t, "us_min_max": [1e6 * v for v in span],
            "bytes_per_s": nbytes / t, "share_of_hbm_peak_8TBps": nbytes / t / HBM_PEAK, "copy_same_bytes_us": 1e6 * t_copy,
            "copy_share_of_hbm_peak_8TBps": nbytes / t_copy / HBM_PEAK, "kernel_over_copy": t / t_copy}


def bench_kernels(groups, dev):
    L, out = _lib.lib(), []
    st = _lib.current_stream(dev)
    for H, W in SIZES:
        for layout in ("yuv420p", "yuv444p"):
            P = 3 * H * W if layout == "yuv444p" else 3 * H * W // 2          # floats of a plane buffer
            img = 12 * H * W
            # ---- the transform, two-view form with the averaged frame
            fwd_bytes, bwd_bytes = 2 * img + 4 * P + img, 4 * P + 2 * img
            sets = max(2, -(-CACHE // fwd_bytes))
            f = [torch.rand(3, H, W, device=dev) for _ in range(sets)]
            b = [torch.rand(3, H, W, device=dev) for _ in range(sets)]
            planes = [torch.empty(P, device=dev) for _ in range(sets)]
            avg = [torch.empty(3, H, W, device=dev) for _ in range(sets)]
            lid, mid = LAYOUTS[layout], MATRICES["bt709"]

            def fwd(k):
                i = k % sets
                _lib.check(L.gsvc_yuv_planes_forward(f[i].data_ptr(), b[i].data_ptr(), H, W, lid, mid, planes[i].data_ptr(), avg[i].data_ptr(), st),
                           "gsvc_yuv_planes_forward")

            def bwd(k):
                i = k % sets
                _lib.check(L.gsvc_yuv_planes_backward(planes[i].data_ptr(), H, W, lid, mid, f[i].data_ptr(), b[i].data_ptr(), st),
                           "gsvc_yuv_planes_backward")
            t, tc, span = alternated(fwd, fwd_bytes, groups, dev)
            out.append(report("k_yuv_planes_fwd", H, W, layout, fwd_bytes, t, tc, span))
            t, tc, span = alternated(bwd, bwd_bytes, groups, dev)          # (overwrites f and b: they are outputs here)
            out.append(report("k_yuv_planes_bwd", H, W, layout, bwd_bytes, t, tc, span))
            del f, b, planes, avg
            torch.cuda.empty_cache()
        # ---- sample codes -> planes, 4:2:0, 8 frames per launch
        for depth in (8, 10):
            fmt = FrameFormat("yuv420p", depth=depth)
            n, nb = 8, frame_bytes(H, W, fmt)
            P = H * W * 3 // 2
            total = n * (nb + 4 * P)
            sets = max(2, -(-CACHE // total))
            codes = [torch.randint(0, 256 if depth == 8 else 4, (n, nb), dtype=torch.uint8, device=dev) for _ in range(sets)]
            outs = [torch.empty(n, P, device=dev) for _ in range(sets)]

            def planes_of(k):
                yuv_loss.frame_planes(codes[k % sets], H, W, fmt, out=outs[k % sets])
            t, tc, span = alternated(planes_of, total, groups, dev)
            r = report("k_frames_planes" + ("16" if depth > 8 else ""), H, W, f"{fmt.name} x {n} frames", total, t, tc, span)
            r["us_per_frame"] = r["us"] / n
            out.append(r)
            del codes, outs
            torch.cuda.empty_cache()
    return out


def torch_planes(f, b, layout, k):
    """The transform as tensor expressions (BT.709)."""
    a = 0.5 * (f + b.flip(-1))
    R, G, B = a[0], a[1], a[2]
    Y = k[0] * R + k[1] * G + k[2] * B
    Cb, Cr = (B - Y) * k[3] + 0.5, (R - Y) * k[4] + 0.5
    if layout == "yuv420p":
        Cb = torch.nn.functional.avg_pool2d(Cb[None, None], 2)[0, 0]
        Cr = torch.nn.functional.avg_pool2d(Cr[None, None], 2)[0, 0]
    return torch.cat([Y.reshape(-1), Cb.reshape(-1), Cr.reshape(-1)]), a


def bench_torch(groups, dev):
    out = []
    Kr, Kb = 0.2126, 0.0722
    k = (Kr, 1 - Kr - Kb, Kb, 1 / (2 * (1 - Kb)), 1 / (2 * (1 - Kr)))
    for H, W in SIZES:
        layout = "yuv420p"
        P = H * W * 3 // 2
        sets = max(2, -(-CACHE // (36 * H * W)))
        f = [torch.rand(3, H, W, device=dev, requires_grad=True) for _ in range(sets)]
        b = [torch.rand(3, H, W, device=dev, requires_grad=True) for _ in range(sets)]
        g = torch.randn(P, device=dev)

        def t_fwd(i):
            with torch.no_grad():
                torch_planes(f[i % sets], b[i % sets], layout, k)

        def k_fwd(i):
            with torch.no_grad():
                yuv_loss.yuv_planes(f[i % sets], b[i % sets], layout, "bt709")

        def t_both(i):
            p, _ = torch_planes(f[i % sets], b[i % sets], layout, k)
            torch.autograd.grad(p, (f[i % sets], b[i % sets]), g)

        def k_both(i):
            Y, C, _ = yuv_loss.yuv_planes(f[i % sets], b[i % sets], layout, "bt709")
            torch.autograd.grad((Y, C), (f[i % sets], b[i % sets]), (g[:H * W].view(Y.shape), g[H * W:].view(C.shape)))
        res = {"H": H, "W": W, "layout": layout}
        for name, fn_t, fn_k in (("forward", t_fwd, k_fwd), ("forward_backward", t_both, k_both)):
            for _ in range(2):
                timed_group(fn_t, 5)
                timed_group(fn_k, 5)
            tt, tk = [], []
            for _ in range(max(groups // 2, 10)):          # alternated
                tt.append(timed_group(fn_t, 5))
                tk.append(timed_group(fn_k, 5))
            res[name] = {"tensor_expressions_us": 1e6 * statistics.median(tt), "yuv_planes_us": 1e6 * statistics.median(tk),
                         "tensor_over_kernels": statistics.median(tt) / statistics.median(tk)}
        out.append(res)
        del f, b
        torch.cuda.empty_cache()
    return out


def write_clip(path, H, W, T, dev, seed=7):
    """The synthetic video as a yuv420p (BT.709, limited range) Y4M file."""
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import Y4MWriter, frames_to_u8
    cube = SyntheticFrameCube(H, W, T, seed=seed, device=dev)
    fmt = FrameFormat("yuv420p")
    with Y4MWriter(path, W, H, (25, 1), fmt) as sink:
        for t in range(T):
            sink.write(frames_to_u8([cube._image(t)], fmt)[0].cpu())


def library_launches(trainer, it):
    """{kernel: launches} of the library's kernels in one step."""
    torch.cuda.synchronize()
    _lib.profile_enable(1)
    _lib.profile_collect(256)
    trainer.step(it)
    torch.cuda.synchronize()
    counts = {k: v[0] for k, v in _lib.profile_collect(256).items()}
    _lib.profile_enable(0)
    return counts


def bench_step(name, H, W, T, anchors, groups, dev, tmp):
    from gsvc_amd.arguments import cfg_20240919
    from gsvc_amd.fit_setup import configure_fit, new_fit
    from gsvc_amd.frames_in import VideoFileCube
    path = os.path.join(tmp, f"{name}.y4m")
    write_clip(path, H, W, T, dev)
    fits = {}
    for domain in ("rgb", "yuv420"):
        cube = VideoFileCube(path, resident="float", device=dev)
        mp_, opt, pipe = cfg_20240919()
        opt.optical_lambda = 0.0
        configure_fit(mp_, opt, cube, 40_000, 0.004, min(16.0, float(T)), None)          # (the reference's schedule: these steps are full precision)
        opt.loss_domain = domain
        pc, trainer = new_fit(cube, mp_, opt, pipe, anchors, dev)
        fits[domain] = [trainer, 0]

    def run(domain, steps):
        trainer, it = fits[domain]
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            it += 1
            trainer.step(it)
        b.record()
        b.synchronize()
        fits[domain][1] = it
        return a.elapsed_time(b) * 1e-3 / steps
    for domain in fits:
        run(domain, 30)
    times = {d: [] for d in fits}
    for _ in range(groups):          # alternated
        for d in fits:
            times[d].append(run(d, 10))
    launches = {}
    for d in fits:
        fits[d][1] += 1
        launches[d] = library_launches(fits[d][0], fits[d][1])
    added = {k: launches["yuv420"].get(k, 0) - launches["rgb"].get(k, 0) for k in sorted(set(launches["rgb"]) | set(launches["yuv420"]))}
    added = {k: v for k, v in added.items() if v}
    med = {d: statistics.median(v) for d, v in times.items()}
    for trainer, _ in fits.values():
        trainer.close()
    return {"clip": name, "H": H, "W": W, "frames": T, "anchors_init": anchors, "groups": groups, "steps_per_group": 10,
            "ms_per_step": {d: 1e3 * med[d] for d in med}, "ms_per_step_min_max": {d: [1e3 * min(v), 1e3 * max(v)] for d, v in times.items()},
            "yuv420_over_rgb": med["yuv420"] / med["rgb"], "library_launches_per_step": {d: sum(v.values()) for d, v in launches.items()},
            "library_launches_yuv420_minus_rgb": added, "library_launches_added": sum(added.values()),
            "tensor_library_launches_added_from_the_code": {"sums / n (ssim_l1 forward)": 2, "stack of the two upstream gradients (ssim_l1 backward)": 2,
                                                            "cat of gY and gC (yuv_planes backward)": 2}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=30)
    ap.add_argument("--step-frames", type=int, default=16, help="frames of the 1080p synthetic video of the step measurement")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--write-clip", default=None, metavar="PATH.y4m",
                    help="only write the synthetic video of tools/fit_synthetic.py (seed 1234; --height, --width, --frames) as yuv420p and exit: "
                         "the input of the two fits of DESIGN.md section 8i")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--frames", type=int, default=64)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_yuv_loss.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.write_clip:
        write_clip(args.write_clip, args.height, args.width, args.frames, dev, seed=1234)
        print(json.dumps({"tool": "bench_yuv_loss", "wrote": args.write_clip, "H": args.height, "W": args.width, "frames": args.frames}))
        return
    res = {"tool": "bench_yuv_loss", "device": torch.cuda.get_device_name(dev), "groups": max(args.groups, 30), "calls_per_group": 20}
    with torch.no_grad():
        res["kernels"] = bench_kernels(max(args.groups, 30), dev)
    if not args.no_torch:
        res["torch"] = bench_torch(args.groups, dev)
    if not args.no_step:
        with tempfile.TemporaryDirectory() as tmp:
            res["step"] = [bench_step("test_clip_64x48", 48, 64, 8, 3000, max(args.groups // 2, 10), dev, tmp),
                           bench_step("synthetic_1080p", 1080, 1920, args.step_frames, 100_000, max(args.groups // 2, 10), dev, tmp)]
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
