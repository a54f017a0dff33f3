#!/usr/bin/env python3
"""Resample a video file to another size (gsvc_amd/resample.py): the Lanczos-3 resampler on the file's codes that
``gsvc_encode.py --coded-size`` puts in front of its fit and ``gsvc_decode.py --size`` behind its decode, written out as a video in the
source's own format.

    python tools/scale_video.py in.y4m out.y4m --size WxH [--video-size WxH --video-format yuv420p10le,bt709,limited]

Y'CbCr files only; each side changes by a ratio of at most 4 either way; 4:2:0 needs even sizes.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    from gsvc_amd.resample import parse_size          # (the one reader of a WxH option; needs neither torch nor the library)
    ap = argparse.ArgumentParser()
    ap.add_argument("video", help="8-bit or 10 / 12 / 16-bit Y'CbCr video file: .y4m, or raw .yuv with --video-size")
    ap.add_argument("output", help="the resampled video: .y4m or .yuv, in the source's format")
    ap.add_argument("--size", type=parse_size, required=True, metavar="WxH", help="the size of the output")
    ap.add_argument("--video-size", type=parse_size, default=None, metavar="WxH", help="frame size of a raw video file")
    ap.add_argument("--video-format", default=None, metavar="LAYOUT[,MATRIX[,RANGE]]", help="e.g. yuv420p,bt601,full or yuv420p10le")
    args = ap.parse_args(argv)
    if os.path.splitext(args.output)[1].lower() not in (".y4m", ".yuv"):
        ap.error("the output is a .y4m or .yuv file")
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch

    from gsvc_amd.encode_options import parse_frame_format
    from gsvc_amd.resample import resample_video
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    vw, vh = args.video_size or (None, None)
    video_fmt = parse_frame_format(args.video_format) if args.video_format else None
    log = resample_video(args.video, args.output, args.size, W=vw, H=vh, fmt=video_fmt, device=dev)
    log = dict({"output": args.output}, **log)
    print(json.dumps(log))
    return log


if __name__ == "__main__":
    main()
