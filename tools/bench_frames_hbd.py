#!/usr/bin/env python3
"""What the deep (10 / 12 / 16-bit) frame stages cost (the k_frames_*16 kernels of csrc/frames_out.hip and csrc/frames_in.hip).
One process, one JSON line.

  kernel   per size (1080 x 1920, 2160 x 3840), direction (out: float images -> frames; in: frames -> float images), layout (yuv444p,
           yuv420p; in, 4:2:0: both chroma modes) and depth (10, 12, 16), n = 8 frames per launch: device-event time of groups of 20
           launches, median over >= 30 groups, per frame; algorithmic bytes per frame 12 H W + frame_bytes from the shapes; achieved
           bytes/s and its share of the 8 TB/s HBM peak (a KERNEL's share of peak, not an end-to-end rate).  The float side (and, for
           `in`, the frames too) rotates through enough sets to exceed the 256 MiB Infinity Cache, so the traffic is HBM's.
  torch    the same conversion written as the tensor expressions a user would write without the kernel (``view(torch.int16)``, float
           arithmetic, ``avg_pool2d`` / ``F.interpolate``, ``clamp``, ``cat``), same inputs, groups alternated with the kernel's in the
           same process; ratio = torch / kernel.  ``max_code_difference`` / ``max_abs_difference`` say that the two compute the same.
  --headline   additionally fits the headline model of tools/bench_frames_out.py and takes ``report.evaluate`` on unrounded floats and
           on frames delivered as 8-bit and as 10-bit yuv444p.

    python tools/bench_frames_hbd.py [--groups 30] [--sizes 1080x1920,2160x3840] [--headline] [--json profiles/frames_hbd.json]
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


def _constants(fmt: FrameFormat):
    """(y_off, y_scale, c_off, c_scale, top) of code = off + scale * value (include/gsvc_hip.h, gsvc_frames_to_u16)."""
    up, top = float(2 ** (fmt.depth - 8)), float(2 ** fmt.depth - 1)
    if fmt.range == "limited":
        return 16.0 * up, 219.0 * up, 128.0 * up, 224.0 * up, top
    return 0.0, top, 128.0 * up, top, top


def torch_to_frames(images, fmt: FrameFormat):
    """float images -> uint8 [n, frame_bytes] of little-endian 16-bit codes, as tensor expressions."""
    x = torch.stack(images).clamp(0.0, 1.0)
    half = 0.5 if fmt.rounding_used == "nearest" else 0.0
    Kr, Kb = MATRIX[fmt.matrix]
    R, G, B = x[:, 0], x[:, 1], x[:, 2]
    Y = Kr * R + (1.0 - Kr - Kb) * G + Kb * B
    Cb, Cr = (B - Y) / (2.0 * (1.0 - Kb)), (R - Y) / (2.0 * (1.0 - Kr))
    if fmt.layout == "yuv420p":
        Cb = torch.nn.functional.avg_pool2d(Cb.unsqueeze(1), 2).squeeze(1)
        Cr = torch.nn.functional.avg_pool2d(Cr.unsqueeze(1), 2).squeeze(1)
    yo, ys, co, cs, top = _constants(fmt)

    def q(v):          # (through int32: a code above 32767 wraps into the int16 that holds the same 16 bits)
        return v.clamp(0.0, top).add(half).to(torch.int32).to(torch.int16).flatten(1)
    return torch.cat([q(yo + ys * Y), q(co + cs * Cb), q(co + cs * Cr)], 1).view(torch.uint8)


def torch_from_frames(frames, H, W, fmt: FrameFormat, chroma):
    """uint8 [n, frame_bytes] of little-endian 16-bit codes -> float32 [n, 3, H, W], as tensor expressions."""
    n = frames.shape[0]
    codes = (frames.view(torch.int16).to(torch.int32) & 0xFFFF).float()
    ch, cw = (H // 2, W // 2) if fmt.layout == "yuv420p" else (H, W)
    y = codes[:, :H * W].view(n, 1, H, W)
    u = codes[:, H * W:H * W + ch * cw].view(n, 1, ch, cw)
    v = codes[:, H * W + ch * cw:].view(n, 1, ch, cw)
    if fmt.layout == "yuv420p":
        kw = dict(mode="bilinear", align_corners=False) if chroma == "bilinear" else dict(mode="nearest")
        u = torch.nn.functional.interpolate(u, scale_factor=2, **kw)
        v = torch.nn.functional.interpolate(v, scale_factor=2, **kw)
    Kr, Kb = MATRIX[fmt.matrix]
    Kg = 1.0 - Kr - Kb
    yo, ys, co, cs, _ = _constants(fmt)
    Y, Cb, Cr = (y - yo) / ys, (u - co) / cs, (v - co) / cs
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


def _measure(kernel, expr, groups):
    for _ in range(3):
        timed_group(kernel, 20)
        timed_group(expr, 4)
    tk, tt = [], []
    for _ in range(groups):          # alternated
        tk.append(timed_group(kernel, 20))
        tt.append(timed_group(expr, 4))
    return statistics.median(tk), statistics.median(tt), tk


def _row(direction, H, W, fmt, chroma, n, nbytes, groups, k_med, t_med, tk, extra):
    alg = 12 * H * W + nbytes
    row = {"direction": direction, "H": H, "W": W, "layout": fmt.layout, "depth": fmt.depth, "format": fmt.name,
           "chroma": chroma if direction == "in" and fmt.layout == "yuv420p" else None, "n": n, "frame_bytes": nbytes, "groups": groups,
           "launches_per_group": 20, "kernel_us_per_frame": 1e6 * k_med / n, "kernel_us_per_frame_min_max": [1e6 * min(tk) / n, 1e6 * max(tk) / n],
           "algorithmic_bytes_per_frame": alg, "kernel_bytes_per_s": alg * n / k_med, "kernel_share_of_hbm_peak_8TBps": alg * n / k_med / HBM_PEAK,
           "torch_expressions_us_per_frame": 1e6 * t_med / n, "torch_over_kernel": t_med / k_med}
    row.update(extra)
    return row


def bench_out(H, W, fmt, n, groups, dev):
    nbytes = fo.frame_bytes(H, W, fmt)
    sets = max(2, -(-(300 << 20) // (n * 12 * H * W)))          # image sets: together more than the 256 MiB last-level cache
    g = torch.Generator(device=dev).manual_seed(H + fmt.depth)
    inputs = [[torch.rand((3, H, W), device=dev, generator=g) * 1.2 - 0.1 for _ in range(n)] for _ in range(sets)]
    out = torch.empty((n, nbytes), dtype=torch.uint8, device=dev)
    a = fo.frames_to_u8(inputs[0], fmt).view(torch.int16).int() & 0xFFFF
    b = torch_to_frames(inputs[0], fmt).view(torch.int16).int() & 0xFFFF
    same = int((a - b).abs().max())
    k_med, t_med, tk = _measure(lambda k: fo.frames_to_u8(inputs[k % sets], fmt, out=out), lambda k: torch_to_frames(inputs[k % sets], fmt), groups)
    return _row("out", H, W, fmt, None, n, nbytes, groups, k_med, t_med, tk, {"input_sets": sets, "max_code_difference_kernel_vs_torch": same})


def bench_in(H, W, fmt, chroma, n, groups, dev):
    nbytes = fo.frame_bytes(H, W, fmt)
    sets = max(2, -(-(300 << 20) // (n * nbytes)))
    out_sets = max(2, -(-(300 << 20) // (n * 12 * H * W)))
    g = torch.Generator(device=dev).manual_seed(H + fmt.depth)
    inputs = [torch.randint(0, 2 ** fmt.depth, (n, nbytes // 2), dtype=torch.int32, device=dev, generator=g).to(torch.int16).view(torch.uint8)
              for _ in range(sets)]
    outs = [torch.empty((n, 3, H, W), dtype=torch.float32, device=dev) for _ in range(out_sets)]
    diff = float((fi.frames_from_u8(inputs[0], H, W, fmt, chroma) - torch_from_frames(inputs[0], H, W, fmt, chroma)).abs().max())
    k_med, t_med, tk = _measure(lambda k: fi.frames_from_u8(inputs[k % sets], H, W, fmt, chroma, out=outs[k % out_sets]),
                                lambda k: torch_from_frames(inputs[k % sets], H, W, fmt, chroma), groups)
    return _row("in", H, W, fmt, chroma, n, nbytes, groups, k_med, t_med, tk,
                {"input_sets": sets, "output_sets": out_sets, "max_abs_difference_kernel_vs_torch": diff})


def headline(anchors, steps, frames, dev):
    """PSNR of the fitted headline model on unrounded floats and on what a viewer of delivered 8-bit / 10-bit yuv444p frames sees."""
    from bench_frames_out import headline_model
    from gsvc_amd.report import evaluate
    pc, cube, pipe, bg = headline_model(anchors, steps, dev)
    ids = list(range(8, 8 + frames))
    res = {"anchors": int(pc._anchor.shape[0]), "fit_steps": steps, "frames": frames, "H": 1080, "W": 1920,
           "psnr_float": evaluate(pc, cube, pipe, bg, frame_ids=ids)["psnr"]}
    for fmt in (FrameFormat("yuv444p"), FrameFormat("yuv444p", depth=10), FrameFormat("yuv444p", range="full"),
                FrameFormat("yuv444p", range="full", depth=10)):
        res[f"psnr_delivered_{fmt.name}_{fmt.range}"] = evaluate(pc, cube, pipe, bg, frame_ids=ids, delivered=fmt)["psnr"]
    res["psnr_eight_bit_rgb24_trunc"] = evaluate(pc, cube, pipe, bg, frame_ids=ids, eight_bit=True)["psnr"]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=30)
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    ap.add_argument("--depths", default="10,12,16")
    ap.add_argument("--headline", action="store_true")
    ap.add_argument("--anchors", type=int, default=245_000)
    ap.add_argument("--fit-steps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_frames_hbd.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "bench_frames_hbd", "device": torch.cuda.get_device_name(dev), "kernel": []}
    groups = max(args.groups, 30)
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        for depth in (int(d) for d in args.depths.split(",")):
            for layout in ("yuv444p", "yuv420p"):
                fmt = FrameFormat(layout, depth=depth)
                with torch.no_grad():
                    res["kernel"].append(bench_out(H, W, fmt, 8, groups, dev))
                    torch.cuda.empty_cache()
                    for chroma in (("bilinear", "nearest") if layout == "yuv420p" else ("bilinear",)):
                        res["kernel"].append(bench_in(H, W, fmt, chroma, 8, groups, dev))
                        torch.cuda.empty_cache()
    if args.headline:
        res["headline"] = headline(args.anchors, args.fit_steps, args.frames, dev)
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
