#!/usr/bin/env python3
"""Decode a bitstream file (tools/gsvc_encode.py; gsvc_amd/bitstream.py) to a video.  The file is all it reads:

    python tools/gsvc_decode.py clip.gsvc -o out.y4m [--format yuv420p10le] [--no-verify | --strict] [--no-film-grain]
                                [--size display|coded|WxH]
    python tools/gsvc_decode.py long.gsvs -o part.y4m --frames 300:364

The file is a bitstream file (magic GSVC) or a sequence file of several groups of pictures (magic GSVS; gsvc_amd/sequence.py, DESIGN.md
section 8h), decoded GOP by GOP with one GOP's model resident.  --frames A:B decodes the frames A .. B - 1 alone: only the GOPs that
hold them are read and built.

-o: .y4m / .yuv (yuv420p unless --format says otherwise), .rgb (rgb24), else a directory of PNGs.  The picture hash of every frame is
taken on the device and, where the file carries hashes of the format decoded to, compared: the JSON line printed says how many frames
were verified and which did not match.  --strict: exit status 1 on a mismatch, or when nothing could be verified.  A file with
film-grain parameters (section GRAN) has its grain synthesised on the delivered frames, behind the hashes, which stay those of the
ungrained pictures; --no-film-grain delivers the pictures as they are.  --size: "display" (the default) delivers the size the file asks
for — that of its DISP section when it was coded at a reduced size (``gsvc_encode.py --coded-size``), else the coded size —, "coded"
the size the model renders at, WxH any size within a ratio of 4 per side of the coded one, for any file (a preview decode).  The
pictures are resampled on the device (gsvc_amd/resample.py) behind the hashes, which are those of the coded-size
pictures; an rgb24 output gets the coded size.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse_args(argv=None):
    from gsvc_amd.resample import parse_decode_size          # (needs neither torch nor the library)
    ap = argparse.ArgumentParser()
    ap.add_argument("bitstream")
    ap.add_argument("-o", "--output", required=True, metavar="PATH")
    ap.add_argument("--format", default=None, metavar="LAYOUT[,MATRIX[,RANGE]]",
                    help="e.g. yuv420p10le or yuv444p,bt709,full (default: the format of the file's picture hashes where the output takes it, "
                         "else what the output's extension means)")
    ap.add_argument("--batch", type=int, default=8, help="frames per render batch")
    ap.add_argument("--frames", default=None, metavar="A:B", help="decode the frames A .. B - 1 only (default: all)")
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument("--no-verify", action="store_true", help="do not take picture hashes")
    mode.add_argument("--strict", action="store_true", help="fail when a frame's picture hash differs from the file's, or nothing could be verified")
    ap.add_argument("--no-film-grain", action="store_true", help="do not synthesise the file's film grain (section GRAN) on the frames")
    ap.add_argument("--size", type=parse_decode_size, default="display", metavar="{display,coded,WxH}",
                    help="the size delivered: the file's display size (default), the coded size, or any WxH within a ratio of 4 per side")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    from gsvc_amd.bitstream import BitstreamError, delivered_size
    from gsvc_amd.encode_options import parse_frame_format
    from gsvc_amd.frames_out import FrameFormat, open_sink
    from gsvc_amd.sequence import decode_sequence, open_sequence
    frames = None
    if args.frames:
        try:
            a, b = args.frames.split(":")
            frames = (int(a), int(b))
        except ValueError:
            raise SystemExit(f"--frames is A:B (got {args.frames!r})") from None
    try:
        seq = open_sequence(args.bitstream)
        hash_format = seq.hash_format
    except BitstreamError as e:
        print(f"gsvc_decode: {args.bitstream}: {e}", file=sys.stderr)
        return 2
    fmt, ext = None, os.path.splitext(args.output)[1].lower()
    if args.format:
        fmt = parse_frame_format(args.format)
    elif hash_format is not None:
        takes = {".y4m": ("yuv420p", "yuv444p"), ".yuv": ("yuv420p", "yuv444p"), ".rgb": ("rgb24",)}.get(ext, ("rgb24",))
        if hash_format.layout in takes:
            fmt = hash_format
    if frames is not None and not 0 <= frames[0] < frames[1] <= seq.frames:
        raise SystemExit(f"--frames {args.frames}: not a non-empty range inside the file's {seq.frames} frames")
    will = fmt or FrameFormat("yuv420p" if ext in (".y4m", ".yuv") else "rgb24")          # (what open_sink picks for a format not given)
    try:
        out_W, out_H = delivered_size((seq.W, seq.H), seq.display, args.size, will, "gsvc_decode")
    except BitstreamError as e:
        print(f"gsvc_decode: {args.bitstream}: {e}", file=sys.stderr)
        return 2
    except ValueError as e:
        raise SystemExit(f"--size: {e}") from None
    sink, fmt = open_sink(args.output, out_W, out_H, fps=tuple(seq.fps), fmt=fmt)
    try:
        res = decode_sequence(seq, sink, fmt=fmt, batch=args.batch, verify=not args.no_verify, strict=args.strict, frames=frames,
                              film_grain=not args.no_film_grain, size=(out_W, out_H))
    except BitstreamError as e:
        print(f"gsvc_decode: {args.bitstream}: {e}", file=sys.stderr)
        return 1
    res.pop("hashes", None)
    print(json.dumps(dict(res, output=args.output, file_bytes=seq.file_bytes)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
