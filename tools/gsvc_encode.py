#!/usr/bin/env python3
"""Encode a video file into ONE bitstream file (gsvc_amd/bitstream.py) that tools/gsvc_decode.py turns back into
the video in another process, with nothing else:

    python tools/gsvc_encode.py clip.y4m -o clip.gsvc [--steps 2000 --lmbda 0.004 --anchors 100000 --estimate-flow]
                                [--video-format yuv420p,bt601,full] [--video-size WxH] [--hash-format yuv420p]
                                [--loss-domain rgb|yuv420|yuv444] [--distortion ssim|ms_ssim] [--init detail [--init-cell 8 --init-mix 0.25]]
                                [--film-grain [--film-grain-gain 1.0 --film-grain-seed N]] [--denoise auto|SIGMA [--denoise-gain 1.0]]
                                [--coded-size WxH]
    python tools/gsvc_decode.py clip.gsvc -o out.y4m --strict
    python tools/gsvc_encode.py long.y4m -o long.gsvs --gop-frames 32 [--scene-cuts --cut-threshold 0.5 --min-gop 4]

VideoFileCube (optionally with the flow estimated from the frames) -> the fit (the schedule and set-up of tools/fit_synthetic.py:
gsvc_amd/fit_setup.py) -> conduct_stream_encoding with 8-bit MLPs -> the file.  The file is then read back and decoded into a null sink
by the function, batch size and format the decoder will use (``decode_video``), which yields the picture hashes; the file is rewritten
with them (section PHSH).  With --film-grain the grain the fit removed is measured against the source and a few dozen bytes of
parameters are added (section GRAN; gsvc_amd/grain.py): the decoder synthesises grain from them on its frames.
With --denoise the fit is given the motion-compensated temporally filtered source (gsvc_amd/tfilter.py; per GOP
with --gop-frames); the grain statistics of --film-grain are still taken against the original.  With --coded-size WxH the fit is given the
source resampled to that size (gsvc_amd/resample.py; per GOP with --gop-frames; after --denoise), the file says
which size to display (section DISP, the same in every GOP; SEQH and every HEAD carry the coded size) and the decoder resamples its
pictures back; the log's "display" entry says what the delivered pictures keep of the source, and bpp is then taken over DISPLAY
pixels.  YUV sources only, not with --flow-dir or --film-grain.  Prints one JSON line: bytes per section, the file's size, and bpp = 8 x FILE SIZE / (H W T).

With --gop-frames the clip is cut into groups of pictures (GOPs) of at most that many frames (gsvc_amd/scene.py, ``plan_gops``; with
--scene-cuts also where the luma histogram of the frames changes), every GOP is fitted and verified on its own (``fit_setup.encode_gop``;
--steps and --anchors are per GOP) and the GOPs are written as ONE sequence file (magic GSVS; gsvc_amd/sequence.py, DESIGN.md section
8h), also when the plan has one GOP.  The JSON line then lists the GOPs.  Without --gop-frames the file written is the GSVC file.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    from gsvc_amd.encode_options import add_fit_arguments, check_fit_arguments          # (needs neither torch nor the library)
    from gsvc_amd.resample import parse_size
    ap = argparse.ArgumentParser()
    ap.add_argument("video", help="8-bit or 10 / 12 / 16-bit video file: .y4m, or raw .yuv / .rgb with --video-size")
    ap.add_argument("-o", "--output", required=True, metavar="PATH", help="the bitstream file to write (.gsvc)")
    add_fit_arguments(ap)
    ap.add_argument("--hash-format", default="yuv420p", metavar="LAYOUT[,MATRIX[,RANGE]]",
                    help="the frame format whose picture hashes the file carries: what the decoder verifies when it decodes to it")
    ap.add_argument("--gop-frames", type=int, default=None, metavar="N",
                    help="cut the clip into groups of pictures of at most N frames and write a sequence file (GSVS)")
    ap.add_argument("--scene-cuts", action="store_true", help="with --gop-frames: also start a GOP where the luma histogram changes")
    ap.add_argument("--cut-threshold", type=float, default=None, metavar="X",
                    help="histogram distance in [0, 1] above which a frame starts a scene (default 0.5: a starting value, not measured)")
    ap.add_argument("--min-gop", type=int, default=None, metavar="M", help="the shortest GOP (default 4); --gop-frames must be at least 2 M")
    ap.add_argument("--film-grain-gain", type=float, default=None, metavar="X", help="with --film-grain: scale the fitted strengths (default 1.0)")
    ap.add_argument("--film-grain-seed", type=int, default=None, metavar="N", help="with --film-grain: the 64-bit seed (default: derived from the file)")
    ap.add_argument("--coded-size", type=parse_size, default=None, metavar="WxH",
                    help="fit the source resampled to this size (Lanczos-3 on the codes, a ratio of at most 4 per side) and let the decoder "
                         "resample back to the source's size (section DISP); YUV sources only, not with --flow-dir or --film-grain")
    args = ap.parse_args(argv)
    check_fit_arguments(ap, args)
    if args.coded_size is not None and (args.flow_dir is not None or args.film_grain):
        ap.error("--coded-size does not go with --flow-dir (those flows are at the source's size) or --film-grain")
    if not args.film_grain and (args.film_grain_gain is not None or args.film_grain_seed is not None):
        ap.error("--film-grain-gain and --film-grain-seed need --film-grain")
    if args.gop_frames is None and (args.scene_cuts or args.cut_threshold is not None or args.min_gop is not None):
        ap.error("--scene-cuts, --cut-threshold and --min-gop need --gop-frames")
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch

    from gsvc_amd.encode_options import options_from_args
    from gsvc_amd.fit_setup import encode_gop
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    opts = options_from_args(args)
    if args.gop_frames is None:
        blob, log = encode_gop(args.video, dev, options=opts)
        with open(args.output, "wb") as f:
            f.write(blob)
        log = dict({"output": args.output}, **log)
        log["total_bytes"] = int(os.path.getsize(args.output))
        shown = log.get("display", log)          # (bits per DISPLAY pixel where the coded picture is a reduced one)
        log["bpp"] = 8.0 * log["total_bytes"] / (shown["H"] * shown["W"] * log["frames"])
        print(json.dumps(log))
        return log

    from gsvc_amd import scene
    from gsvc_amd.frames_in import open_video
    from gsvc_amd.sequence import write_sequence
    header, frames = open_video(args.video, *opts.video_size, opts.video_format)
    H, W, T = int(header["H"]), int(header["W"]), int(frames.shape[0])
    min_gop = scene.DEFAULT_MIN_GOP if args.min_gop is None else args.min_gop
    threshold = scene.DEFAULT_CUT_THRESHOLD if args.cut_threshold is None else args.cut_threshold
    cuts = scene.detect_cuts((header, frames), dev, threshold)[0] if args.scene_cuts else []
    del frames
    plan = scene.plan_gops(T, cuts, args.gop_frames, min_gop)
    cW, cH = args.coded_size or (W, H)          # SEQH and every GOP's HEAD carry the coded size; bpp is taken over display pixels
    flags = scene.gop_cut_flags(plan, cuts)
    blobs, gops, fit_seconds = [], [], 0.0
    for (first, count), cut in zip(plan, flags):
        blob, one = encode_gop(args.video, dev, frame_range=(first, first + count), options=opts)          # (everything of the GOP's fit is released inside)
        blobs.append(blob)
        fit_seconds += one["fit_seconds"]
        gops.append({"first": first, "frames": count, "bytes": len(blob), "bpp": 8.0 * len(blob) / (H * W * count),
                     "fit_seconds": one["fit_seconds"], "cut": int(cut), "anchors_initial": one["anchors_initial"], "anchors_coded": one["anchors_coded"],
                     "sections": one["sections"], **{k: one[k] for k in ("grain", "denoise", "display", "weighting") if k in one}})
    fps = header.get("fps") or (30, 1)
    write_sequence(args.output, blobs, cW, cH, fps, flags)
    log = {"output": args.output, "W": cW, "H": cH, **({"display": {"W": W, "H": H, "filter": "lanczos3"}} if args.coded_size else {}), "frames": T, "steps": args.steps, "fit_seconds": fit_seconds,
           "loss_domain": one["loss_domain"], "loss_matrix": one["loss_matrix"], "distortion": one["distortion"],
           **{k: one[k] for k in ("init", "init_cell", "init_mix") if k in one},
           "hash_format": opts.hash_format.name, "gop_frames": args.gop_frames, "min_gop": min_gop,
           "scene_cuts": cuts if args.scene_cuts else None, "cut_threshold": threshold if args.scene_cuts else None, "gops": gops}
    log["total_bytes"] = int(os.path.getsize(args.output))
    log["bpp"] = 8.0 * log["total_bytes"] / (H * W * T)
    print(json.dumps(log))
    return log


if __name__ == "__main__":
    main()


