#!/usr/bin/env python3
"""Compare a decoded video file with its source on the sample codes: PSNR-Y / -U / -V, their pooled average, the 6:1:1 mean and
MS-SSIM-Y per frame, the means over the frames and the PSNR of the summed squared error (``gsvc_amd.metrics.compare_videos``; the
kernels of csrc/metrics.hip, so it needs the GPU).  Prints one JSON line.

    python tools/compare_video.py ref.y4m dec.y4m [--json out.json]
    python tools/compare_video.py ref.yuv dec.yuv --size 1920x1080 --format yuv420p10le
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("ref")
    ap.add_argument("dec")
    ap.add_argument("--size", default=None, metavar="WxH", help="frame size of raw .yuv / .rgb files")
    ap.add_argument("--format", default=None, metavar="LAYOUT", help="format of raw files in ffmpeg's spelling (yuv420p, yuv444p10le, rgb24, ...)")
    ap.add_argument("--chunk", type=int, default=16, help="frames uploaded at a time")
    ap.add_argument("--no-per-frame", action="store_true", help="leave the per-frame lists out of the line")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    from gsvc_amd.frames_out import FrameFormat
    from gsvc_amd.metrics import compare_videos
    W = H = None
    if args.size:
        try:
            W, H = (int(v) for v in args.size.lower().split("x"))
        except ValueError:
            raise SystemExit(f"--size is WxH (got {args.size!r})")
    fmt = FrameFormat.from_name(args.format) if args.format else None
    res = dict(compare_videos(args.ref, args.dec, W, H, fmt, chunk=args.chunk), ref=args.ref, dec=args.dec)
    if args.no_per_frame:
        res.pop("per_frame")
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
