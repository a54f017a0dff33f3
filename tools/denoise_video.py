#!/usr/bin/env python3
"""Motion-compensated temporal prefilter of a video file (gsvc_amd/tfilter.py): what ``gsvc_encode.py --denoise``
gives its fit, written out as a video in the source's own format.

    python tools/denoise_video.py in.y4m out.y4m [--sigma auto|SIGMA --gain 1.0] [--gop-frames 32 [--scene-cuts --cut-threshold 0.5 --min-gop 4]]
                                  [--video-size WxH --video-format yuv420p10le,bt709,limited] [--chunk 8]

Without --gop-frames the whole file is one range; with it the file is cut as ``gsvc_encode.py`` cuts it (gsvc_amd/scene.py) and every
GOP is filtered on its own, so nothing is averaged across a cut.  Y'CbCr files only.  Prints one JSON line: per range the noise sigma
and strength used and the PSNR-Y of the output against the input.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    from gsvc_amd.tfilter import parse_sigma          # (the one reader of an {auto,SIGMA} option; needs neither torch nor the library)
    ap = argparse.ArgumentParser()
    ap.add_argument("video", help="8-bit or 10 / 12 / 16-bit Y'CbCr video file: .y4m, or raw .yuv with --video-size")
    ap.add_argument("output", help="the filtered video: .y4m or .yuv, in the source's format")
    ap.add_argument("--sigma", type=parse_sigma, default="auto", metavar="{auto,SIGMA}",
                    help="the noise sigma in codes of the file's depth, or 'auto': estimated per range (a starting value: texture reads as noise)")
    ap.add_argument("--gain", type=float, default=1.0, metavar="X", help="scale the filter's strength")
    ap.add_argument("--video-size", default=None, metavar="WxH", help="frame size of a raw video file")
    ap.add_argument("--video-format", default=None, metavar="LAYOUT[,MATRIX[,RANGE]]", help="e.g. yuv420p,bt601,full or yuv420p10le")
    ap.add_argument("--gop-frames", type=int, default=None, metavar="N", help="filter groups of pictures of at most N frames on their own")
    ap.add_argument("--scene-cuts", action="store_true", help="with --gop-frames: also start a GOP where the luma histogram changes")
    ap.add_argument("--cut-threshold", type=float, default=None, metavar="X", help="histogram distance in [0, 1] above which a frame starts a scene")
    ap.add_argument("--min-gop", type=int, default=None, metavar="M", help="the shortest GOP (default 4); --gop-frames must be at least 2 M")
    ap.add_argument("--chunk", type=int, default=8, metavar="K", help="target frames whose flows are resident at once")
    args = ap.parse_args(argv)
    if args.gop_frames is None and (args.scene_cuts or args.cut_threshold is not None or args.min_gop is not None):
        ap.error("--scene-cuts, --cut-threshold and --min-gop need --gop-frames")
    if not args.gain > 0.0:
        ap.error("--gain must be positive")
    if args.chunk < 1:
        ap.error("--chunk must be at least 1")
    if os.path.splitext(args.output)[1].lower() not in (".y4m", ".yuv"):
        ap.error("the output is a .y4m or .yuv file")
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch

    from gsvc_amd.encode_options import parse_frame_format
    from gsvc_amd.resample import parse_size
    from gsvc_amd.tfilter import denoise_video
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    vw, vh = parse_size(args.video_size) if args.video_size else (None, None)          # (the namespace keeps the text)
    video_fmt = parse_frame_format(args.video_format) if args.video_format else None
    ranges = None
    if args.gop_frames is not None:
        from gsvc_amd import scene
        from gsvc_amd.frames_in import open_video
        header, frames = open_video(args.video, vw, vh, video_fmt)
        min_gop = scene.DEFAULT_MIN_GOP if args.min_gop is None else args.min_gop
        threshold = scene.DEFAULT_CUT_THRESHOLD if args.cut_threshold is None else args.cut_threshold
        cuts = scene.detect_cuts((header, frames), dev, threshold)[0] if args.scene_cuts else []
        ranges = [(first, first + count) for first, count in scene.plan_gops(int(frames.shape[0]), cuts, args.gop_frames, min_gop)]
        del frames
    log = denoise_video(args.video, args.output, sigma=args.sigma, gain=args.gain, W=vw, H=vh, fmt=video_fmt, frame_ranges=ranges, device=dev,
                        chunk=args.chunk)
    log = dict({"output": args.output}, **log)
    print(json.dumps(log))
    return log


if __name__ == "__main__":
    main()
