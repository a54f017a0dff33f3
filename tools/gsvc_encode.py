#!/usr/bin/env python3
"""Encode a video file into ONE bitstream file (gsvc_amd/bitstream.py) that tools/gsvc_decode.py turns back into
the video in another process, with nothing else:

    python tools/gsvc_encode.py clip.y4m -o clip.gsvc [--steps 2000 --lmbda 0.004 --anchors 100000 --estimate-flow]
                                [--video-format yuv420p,bt601,full] [--video-size WxH] [--hash-format yuv420p]
    python tools/gsvc_decode.py clip.gsvc -o out.y4m --strict

VideoFileCube (optionally with the flow estimated from the frames) -> the fit (the schedule and set-up of tools/fit_synthetic.py:
gsvc_amd/fit_setup.py) -> conduct_stream_encoding with 8-bit MLPs -> the file.  The file is then read back and decoded into a null sink
by the function, batch size and format the decoder will use (``decode_video``), which yields the picture hashes; the file is rewritten
with them (section PHSH).  Prints one JSON line: bytes per section, the file's size, and bpp = 8 x FILE SIZE / (H W T).
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _frame_format(text):
    """LAYOUT[,MATRIX[,RANGE]] -> FrameFormat; LAYOUT in ffmpeg's spelling (yuv420p, yuv444p10le, rgb24, ...)."""
    from gsvc_amd.frames_out import FrameFormat
    name, *rest = text.split(",")
    if len(rest) > 2:
        raise SystemExit(f"a frame format is LAYOUT[,MATRIX[,RANGE]] (got {text!r})")
    return FrameFormat.from_name(name, **dict(zip(("matrix", "range"), rest)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("video", help="8-bit or 10 / 12 / 16-bit video file: .y4m, or raw .yuv / .rgb with --video-size")
    ap.add_argument("-o", "--output", required=True, metavar="PATH", help="the bitstream file to write (.gsvc)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--lmbda", type=float, default=0.004)
    ap.add_argument("--anchors", type=int, default=100_000)
    ap.add_argument("--slab-frames", type=float, default=16.0, help="z-slab of a render in frames (2 x threshold x scale)")
    ap.add_argument("--densify-grad-threshold", type=float, default=None, help="default: the reference's 5e-4")
    ap.add_argument("--estimate-flow", action="store_true", help="estimate the optical flow from the frames (gsvc_amd.flow.EstimatedFlowCube)")
    ap.add_argument("--flow-dir", default=None, metavar="DIR", help="optical-flow files, one per frame pair")
    ap.add_argument("--video-size", default=None, metavar="WxH", help="frame size of a raw video file")
    ap.add_argument("--video-format", default=None, metavar="LAYOUT[,MATRIX[,RANGE]]", help="e.g. yuv420p,bt601,full or yuv420p10le")
    ap.add_argument("--hash-format", default="yuv420p", metavar="LAYOUT[,MATRIX[,RANGE]]",
                    help="the frame format whose picture hashes the file carries: what the decoder verifies when it decodes to it")
    args = ap.parse_args(argv)

    import torch

    from gsvc_amd.arguments import cfg_20240919
    from gsvc_amd.bitstream import CubeGeometry, NullSink, decode_video, read_bitstream, unpack_sections, with_hashes, write_bitstream
    from gsvc_amd.fit_setup import configure_fit, new_fit
    from gsvc_amd.frames_in import VideoFileCube
    from gsvc_amd.stream_codec import conduct_stream_encoding
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    mp_, opt, pipe = cfg_20240919()
    vw, vh = (int(v) for v in args.video_size.lower().split("x")) if args.video_size else (None, None)
    cube = VideoFileCube(args.video, optical_flow_dir=args.flow_dir, W=vw, H=vh, fmt=_frame_format(args.video_format) if args.video_format else None,
                         device=dev)
    H, W, T = cube.height, cube.width, cube.len_z_frames
    geometry_source = cube
    if args.estimate_flow:
        from gsvc_amd.flow import EstimatedFlowCube
        cube = EstimatedFlowCube(cube, device=dev)
    elif args.flow_dir is None:
        opt.optical_lambda = 0.0
    configure_fit(mp_, opt, cube, args.steps, args.lmbda, args.slab_frames, args.densify_grad_threshold)
    pc, trainer = new_fit(cube, mp_, opt, pipe, args.anchors, dev)
    bg = trainer.background
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(1, args.steps + 1):
        trainer.step(it)
    torch.cuda.synchronize()
    fit_seconds = time.perf_counter() - t0
    trainer.sync_replicas()
    trainer.close()
    with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
        mlp_file = os.path.join(tmp, "mlp.bin")
        pack = conduct_stream_encoding(pc, mlp_file=mlp_file)          # (quantises the MLPs of pc in place: the shipped form)
        with open(mlp_file, "rb") as f:
            mlp_bytes = f.read()
    geometry = CubeGeometry.of(geometry_source, mp_, pipe, bg.tolist())
    write_bitstream(args.output, pc, pack, geometry, mlp_bytes)
    log = {"output": args.output, "W": W, "H": H, "frames": T, "steps": args.steps, "anchors_coded": int(pack.n), "fit_seconds": fit_seconds}
    # the decoder's own path on the file just written: the hashes are those of the pictures IT produces
    del trainer, cube, geometry_source, pc, pack
    fmt = _frame_format(args.hash_format)
    res = decode_video(read_bitstream(args.output), NullSink(), fmt=fmt, verify=True, device=dev)
    with open(args.output, "rb") as f:
        blob = with_hashes(f.read(), fmt, res["hashes"])
    with open(args.output, "wb") as f:
        f.write(blob)
    log["hash_format"], log["verify_decode_fps"] = fmt.name, res["fps"]
    log["sections"] = {t.decode("ascii"): len(p) for t, p in unpack_sections(blob)}
    log["total_bytes"] = int(os.path.getsize(args.output))
    log["bpp"] = 8.0 * log["total_bytes"] / (H * W * T)
    print(json.dumps(log))
    return log


if __name__ == "__main__":
    main()
