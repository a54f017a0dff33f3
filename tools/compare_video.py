#!/usr/bin/env python3
"""Compare a decoded video file with its source on the sample codes: PSNR-Y / -U / -V, their pooled average, the 6:1:1 mean and
MS-SSIM-Y per frame, the means over the frames and the PSNR of the summed squared error (``gsvc_amd.metrics.compare_videos``; the
kernels of csrc/metrics.hip, so it needs the GPU).  Prints one JSON line.

    python tools/compare_video.py ref.y4m dec.y4m [--json out.json]
    python tools/compare_video.py ref.yuv dec.yuv --size 1920x1080 --format yuv420p10le
    python tools/compare_video.py a.y4m b.y4m --hash      (also each file's per-frame picture hashes, ``metrics.picture_hash``, and whether they agree)
    python tools/compare_video.py ref.y4m dec.y4m --weights w.npy --weight-cell 8      (also wPSNR-Y under the maps of w.npy, gsvc_amd/wdist.py)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _hashes(path, W, H, fmt, chunk):
    """The picture hashes of a video file's frames: [[16 hex digits per plane] per frame]."""
    import torch

    from gsvc_amd.frames_in import open_video
    from gsvc_amd.metrics import picture_hash
    hdr, frames = open_video(path, W, H, fmt)
    out = []
    for i in range(0, int(frames.shape[0]), chunk):
        import numpy as np
        on_dev = torch.from_numpy(np.ascontiguousarray(frames[i:i + chunk])).cuda()
        got = picture_hash(on_dev, hdr["H"], hdr["W"], hdr["fmt"]).cpu().numpy().view(np.uint64)
        out += [[f"{int(v):016x}" for v in row] for row in got]
    return out


def _wpsnr(ref, dec, W, H, fmt, chunk, weights_path, cell):
    """wPSNR-Y of two video files under the weight maps of a .npy ([Hc, Wc] or [frames, Hc, Wc]): {"wpsnr_y": per frame, "wpsnr_y_seq"}."""
    import numpy as np
    import torch

    from gsvc_amd.frames_in import open_video
    from gsvc_amd.wdist import block_sse, load_weights, weighted_psnr_y
    ha, fa = open_video(ref, W, H, fmt)
    hb, fb = open_video(dec, int(ha["W"]), int(ha["H"]), ha["fmt"])
    if fa.shape != fb.shape:
        raise SystemExit(f"--weights: the files differ in frames or size ({tuple(fa.shape)} and {tuple(fb.shape)})")
    h, w, f = int(ha["H"]), int(ha["W"]), ha["fmt"]
    maps = load_weights(weights_path, int(fa.shape[0]), h, w, cell)
    sse = []
    for i in range(0, int(fa.shape[0]), chunk):
        a, b = (torch.from_numpy(np.ascontiguousarray(x[i:i + chunk])).cuda() for x in (fa, fb))
        sse.append(block_sse(a, b, h, w, f, cell).cpu())
    per, pooled = weighted_psnr_y(torch.cat(sse), maps, f.depth, h, w)
    return {"wpsnr_y": [float(v) for v in per], "wpsnr_y_seq": pooled, "weight_cell": cell}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("ref")
    ap.add_argument("dec")
    ap.add_argument("--size", default=None, metavar="WxH", help="frame size of raw .yuv / .rgb files")
    ap.add_argument("--format", default=None, metavar="LAYOUT", help="format of raw files in ffmpeg's spelling (yuv420p, yuv444p10le, rgb24, ...)")
    ap.add_argument("--chunk", type=int, default=16, help="frames uploaded at a time")
    ap.add_argument("--no-per-frame", action="store_true", help="leave the per-frame lists out of the line")
    ap.add_argument("--hash", action="store_true",
                    help="also print the per-frame, per-plane picture hashes of both files (what a bitstream file's PHSH section holds) and whether they agree")
    ap.add_argument("--weights", default=None, metavar="FILE.npy",
                    help="also print wPSNR-Y under these weight maps ([Hc, Wc] or [frames, Hc, Wc]; normalised per frame; YUV files only)")
    ap.add_argument("--weight-cell", type=int, choices=(4, 8, 16), default=8, metavar="N", help="the cell of --weights in pixels (default 8)")
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
    if args.hash:
        ha, hb = _hashes(args.ref, W, H, fmt, max(1, args.chunk)), _hashes(args.dec, W, H, fmt, max(1, args.chunk))
        same = [a == b for a, b in zip(ha, hb)]
        res["picture_hash"] = {"ref": ha, "dec": hb, "equal": same, "all_equal": all(same)}
    if args.weights:
        wp = _wpsnr(args.ref, args.dec, W, H, fmt, max(1, args.chunk), args.weights, args.weight_cell)
        res["wpsnr_y_seq"], res["weight_cell"] = wp["wpsnr_y_seq"], wp["weight_cell"]
        res["per_frame"]["wpsnr_y"] = wp["wpsnr_y"]
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
