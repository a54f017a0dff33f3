"""The set-up of a fit that tools/fit_synthetic.py and tools/gsvc_encode.py share: the reference's 40 000-iteration schedule scaled to
a run's length, the model, its initial anchors and the Trainer on a frame cube, and ``encode_gop``: a range of frames of a video file
fitted, stream-encoded and verified into the bytes of one bitstream file (a whole clip, or one group of pictures of a sequence file).

The reference's schedule (pipeline/train.py:325-583: 10 k full precision / 5 k quantised / 20 k entropy-constrained / 5 k
straight-through; statistics from 500, densification 1 500 .. 25 000 every 100, paused 1 000 iterations at the first phase change) is
scaled to ``steps`` iterations with the same proportions.

``encode_gop`` takes one ``encode_options.EncodeOptions`` and runs these stages in this order, each a function below; the measures decode
through ``decoded_batches`` and open the file again through ``source_range``, and ``release`` returns a stage's device memory before the next:

    stage              what it does                                                                   the log keys it writes
    prepare_source     denoise, coded_size: the prefilter at source size, then the resampler          "denoise" (stands behind "steps")
    source_cube        the VideoFileCube of those frames, or of the file's own
    fit_gop            flow, schedule, new_fit, the steps, conduct_stream_encoding -> the file image  "W" "H" "frames" "steps" "init" ("init_cell" "init_mix")
                                                                                                      "anchors_initial" "loss_domain" "loss_matrix" "distortion"
                                                                                                      "fit_seconds" "anchors_coded"
    verify_decode      the decoder's own path on the image; its hashes become the section PHSH        "hash_format" "verify_decode_fps"
    measure_weighting  a weighted fit: one more decode against the frames the fit saw                 "weighting"
    measure_display    coded_size: the section DISP, one more decode at display size                  "display"
    measure_grain      film_grain: one more decode against the source, the section GRAN               "grain"
    encode_gop         the section sizes of the final image                                           "sections"
"""
from __future__ import annotations

import numpy as np
import torch


def configure_fit(mp_, opt, cube, steps: int, lmbda: float, slab_frames: float, densify_grad_threshold=None):
    """Set the render slab (``mp_.threshold``: ``slab_frames`` frames thick) and scale the schedule of ``opt`` to ``steps`` iterations,
    in place."""
    N = int(steps)
    mp_.threshold = slab_frames / 2.0 / cube.scale
    s = N / 40_000.0
    opt.iterations, opt.lmbda = N, lmbda
    opt.full_precision_training_total, opt.quantized_training_total = int(10_000 * s), int(5_000 * s)
    opt.entropy_constrained_train_total = int(20_000 * s)
    opt.ste_entropy_constrained_train_total = N - int(35_000 * s)
    opt.start_stat, opt.update_from, opt.update_until = int(500 * s), int(1_500 * s), int(25_000 * s)
    opt.update_interval = max(20, int(100 * s))
    opt.pause_densification = int(1_000 * s)
    if densify_grad_threshold is not None:
        opt.densify_grad_threshold = densify_grad_threshold
    for name in dir(opt):                        # the learning-rate schedules decay over the run's length
        if name.endswith("_max_steps"):
            setattr(opt, name, N)


def new_fit(cube, mp_, opt, pipe, anchors: int, device, init: str = "uniform", init_cell: int = 8, init_mix: float = 0.25,
            weighting=None, weight_strength: float = 0.5, weight_cell=None, roi=None, weight_file=None, roi_base_hw=None):
    """Seed the generators, build the model of configuration ``mp_`` with ``anchors`` initial points and its Trainer -> ``(pc, trainer)``.
      ``init="uniform"``  the points are drawn uniformly inside the cube (reference frame_cube/utils.py:6-15, init_point_cloud, bleed 0.1).
      ``init="detail"``   they are drawn where the clip's luma has detail (gsvc_amd/detail.py, ``detail_points``: cells of ``init_cell``
                          pixels, a share ``init_mix`` of the points uniform; both defaults are starting values, not measured ones).
    Either way ``create_from_points`` merges the points of a voxel and sets every anchor's scale from its 3-NN distance.
      ``weighting="activity"``, ``roi=[(x, y, w, h, weight), ...]``, ``weight_file``: spatially weighted distortion (gsvc_amd/wdist.py,
                          ``fit_weights``: cells of ``weight_cell`` pixels, None = 8; ``weight_strength`` of the activity map; rectangles in
                          the pixels of ``roi_base_hw = (H, W)``, None = the cube's).  The maps are built on the cube's own frames before
                          anything is seeded, and the Trainer carries them (``trainer.weight_maps`` on the device, ``trainer.weighting``:
                          what a log says of them).  Without these arguments nothing changes and ``trainer.weighting`` is None."""
    from . import detail, wdist
    maps, weighting_info = wdist.fit_weights(cube, weighting, weight_strength, weight_cell, roi, weight_file, roi_base_hw=roi_base_hw)
    if init not in detail.INITS:
        raise ValueError(f"new_fit: init must be one of {', '.join(detail.INITS)} (got {init!r})")
    if init == "detail":
        init_cell, init_mix = detail.check_cell_mix(init_cell, init_mix, "new_fit")
    from . import dist as gdist
    from .model import GaussianModel
    from .train import Trainer
    torch.manual_seed(0)
    np.random.seed(0)
    pc = GaussianModel(mp_, mp_.anchor_feature_dim, mp_.n_offsets, mp_.voxel_size, mp_.update_depth, mp_.update_init_factor,
                       mp_.update_hierarchy_factor, mp_.use_feat_bank, n_features_per_level=mp_.grid_feature_dim,
                       log2_hashmap_size=mp_.log2, log2_hashmap_size_2D=mp_.log2_2D, device=device)
    if init == "detail":
        points, _ = detail.detail_points(cube, anchors, init_cell, init_mix, seed=0)
        pc.create_from_points(points, spatial_lr_scale=1.0)
    else:
        lim = np.array([cube.x_min, cube.y_min, cube.z_min]) * 1.1
        pc.create_from_points(np.random.default_rng(0).uniform(lim, -lim, (anchors, 3)), spatial_lr_scale=1.0)
    pc.update_anchor_bound(cube.x_min, cube.y_min, cube.z_min)
    pc.training_setup(opt)
    gdist.broadcast_parameters(pc)
    trainer = Trainer(pc, cube, opt, pipe, mp_, seed=0, weight_maps=maps, weight_cell=weighting_info and weighting_info["cell"])
    trainer.weighting = weighting_info
    return pc, trainer


def decoded_batches(bs, fmt, device, batch: int = 8, out_size=None):
    """Decode ``bs`` (a parsed ``Bitstream``) into ``fmt`` on the device, render batch by render batch (``render_frames_u8`` with
    ``to_host=False``; at ``out_size = (H, W)`` when given) -> a generator of ``(first_frame, rows)``, ``rows`` uint8 ``[n, frame_bytes]``
    on the device.  ``batch`` is the render batch: a frame's bits depend on whether it was rendered in a batch of one."""
    from .frames_out import render_frames_u8
    pc, cams, pipe, bg = bs.build_model(device)
    frames = render_frames_u8(cams, pc, pipe, bg, fmt=fmt, batch=int(batch), to_host=False, out_size=out_size)
    try:
        for first in range(0, len(cams), int(batch)):
            with torch.no_grad():          # (around the render alone: a generator must not leave the mode on for its caller)
                rows = torch.stack([next(frames) for _ in range(min(int(batch), len(cams) - first))])
            yield first, rows
    finally:
        with torch.no_grad():          # (the render loop restores the mode it started in when it ends: it ends here, not when collected)
            frames.close()


def decoded_against(bs, source_frames, fmt, device, what: str, batch: int = 8, out_size=None, has: str = "the source has"):
    """``decoded_batches`` paired with the source's codes -> a generator of ``(rows, source rows)``: ``source_frames`` is the host array
    ``[T, frame_bytes]`` of ``frames_in.open_video``, uploaded a batch at a time.  A ``ValueError`` at the end when the file decodes to
    another number of frames than ``source_frames`` has."""
    got, T = 0, int(source_frames.shape[0])
    for first, rows in decoded_batches(bs, fmt, device, batch, out_size):
        got = first + int(rows.shape[0])
        yield rows, torch.from_numpy(np.ascontiguousarray(source_frames[first:got])).to(rows.device)
    if got != T:
        raise ValueError(f"{what}: the file decodes to {got} frames, {has} {T}")


def grain_statistics(bs, source_frames, H: int, W: int, fmt, device, batch: int = 8, flat_threshold=None, max_residual=None):
    """The film-grain statistics of a file image against its source: ``bs`` is decoded into ``fmt``, the SOURCE's own format, each
    batch's ``grain.grain_stats`` against the source's codes is taken on the device, and the batches are summed on the host as Python
    ints -> nested lists ``[3][16][6]``.  ``flat_threshold``, ``max_residual``: the two rejection thresholds of ``grain.grain_stats``
    (None: its defaults, which are starting values)."""
    from .grain import BINS, DEFAULT_FLAT_THRESHOLD, DEFAULT_MAX_RESIDUAL, grain_stats
    flat = DEFAULT_FLAT_THRESHOLD if flat_threshold is None else int(flat_threshold)
    worst = DEFAULT_MAX_RESIDUAL if max_residual is None else int(max_residual)
    parts = [grain_stats(src, rows, H, W, fmt, flat_threshold=flat, max_residual=worst).cpu().tolist()
             for rows, src in decoded_against(bs, source_frames, fmt, device, "grain_statistics", batch)]
    return [[[sum(part[p][b][j] for part in parts) for j in range(6)] for b in range(BINS)] for p in range(3)]


def display_psnr(bs, source_frames, fmt, device, batch: int = 8):
    """What a reduced-resolution file delivers against its source: ``bs`` (with a DISP section) is decoded into ``fmt``, the SOURCE's own
    format, at display size, and each batch's ``metrics.plane_sse`` against the source's codes (``source_frames`` at display size) is
    summed over all frames -> ``(psnr_y, psnr_611)``, the latter ``(6 Y + U + V) / 8`` of the three plane PSNRs."""
    from .metrics import plane_samples, plane_sse, psnr_of_sse
    W, H = bs.display_size
    total = torch.zeros(3, dtype=torch.int64, device=device)
    out_size = None if (W, H) == tuple(bs.coded_size) else (H, W)
    for rows, src in decoded_against(bs, source_frames, fmt, device, "display_psnr", batch, out_size):
        total += plane_sse(rows, src, H, W, fmt).sum(dim=0)
    samples = torch.tensor(plane_samples(H, W, fmt), dtype=torch.float64, device=total.device) * int(source_frames.shape[0])
    p = [float(v) for v in psnr_of_sse(total, samples, float((1 << fmt.depth) - 1)).tolist()]
    return p[0], (6.0 * p[0] + p[1] + p[2]) / 8.0


def coded_wpsnr(bs, fit_frames, fmt, weight_maps, cell: int, device, batch: int = 8):
    """What a weighted fit bought, on the delivered codes: ``bs`` is decoded into ``fmt``, the format of the frames the fit was given, at
    the size it was fitted at, and each batch's ``wdist.block_sse`` against those frames (``fit_frames``) is kept -> ``(psnr_y, wpsnr_y)``
    pooled over the frames: the plain luma PSNR and ``wdist.weighted_psnr_y`` under ``weight_maps`` ``[T, Hc, Wc]``."""
    from .wdist import block_sse, weighted_psnr_y
    W, H = bs.coded_size
    sse = torch.cat([block_sse(rows, src, H, W, fmt, cell).cpu()
                     for rows, src in decoded_against(bs, fit_frames, fmt, device, "coded_wpsnr", batch, has="the fit saw")])
    _, plain = weighted_psnr_y(sse, torch.ones(sse.shape, dtype=torch.float64), fmt.depth, H, W)
    _, weighted = weighted_psnr_y(sse, weight_maps, fmt.depth, H, W)
    return plain, weighted


def release():
    """Return what a finished stage held to the device: unreachable objects are collected and the allocator's cache is emptied."""
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def source_range(video, frame_range, options):
    """The frames ``frame_range = (first, stop)`` (None: all) of the video file as it is -> ``(header, host array [T, frame_bytes])`` of
    ``frames_in.open_video`` (memory-mapped: a stage that needs them opens the file again).  ``ValueError``: no non-empty range inside it."""
    from .frames_in import open_video
    hdr, source = open_video(video, options.video_size[0], options.video_size[1], options.video_format)
    if frame_range is None:
        return hdr, source
    try:
        first, stop = (int(v) for v in frame_range)
    except (TypeError, ValueError):
        raise ValueError(f"encode_gop: frame_range must be (first, stop) (got {frame_range!r})") from None
    if not 0 <= first < stop <= int(source.shape[0]):          # (what VideoFileCube refuses, before anything is filtered)
        raise ValueError(f"encode_gop: frame_range ({first}, {stop}) is not a non-empty range inside the {int(source.shape[0])} "
                         f"frames of {video}")
    return hdr, source[first:stop]


def prepare_source(video, device, frame_range, options):
    """``denoise`` and ``coded_size`` -> ``(frames, coded_size, display_size, denoise_log)``.  The frames of ``frame_range`` are put through
    the motion-compensated temporal prefilter at the source's size (``tfilter.denoise_range`` with ``denoise_gain``; one range, so
    nothing is filtered across its ends), then resampled on the device to the coded size in the source's own format
    (``resample.resample_range``): ``frames`` is the host array the fit is to be given, ``coded_size`` and ``display_size`` its and the
    source's ``(W, H)``.  Each is None where its option is off; with both off the file is not opened.  A ``ValueError`` before anything is
    filtered: an ``rgb24`` source, and what ``resample.check_sizes`` refuses (a ratio above 4, an odd size for 4:2:0).
    Log entry: "denoise": {"sigma", "q", "source", "gain", "psnr_y"}, handed on as ``denoise_log``."""
    frames, denoise_log, size = None, None, options.frame_size
    if options.denoise is None and size is None:
        return None, None, None, None
    hdr, source = source_range(video, frame_range, options)
    H, W, fmt = int(hdr["H"]), int(hdr["W"]), hdr["fmt"]
    if fmt.layout == "rgb24":
        raise ValueError("encode_gop: the temporal prefilter and the resampler work on Y'CbCr codes; an rgb24 source has none")
    if size is not None:
        from .resample import check_sizes, resample_range
        check_sizes(H, W, size[1], size[0], fmt, "encode_gop: coded_size")
    if options.denoise is not None:
        from .tfilter import denoise_range
        frames, denoise_log = denoise_range(source, H, W, fmt, device, sigma=options.denoise, gain=float(options.denoise_gain))
    if size is not None:
        frames = resample_range(source if frames is None else frames, H, W, fmt, size[1], size[0], device)
    return frames, size, (W, H) if size is not None else None, denoise_log


def source_cube(video, device, frame_range, options, frames=None, coded_size=None):
    """The ``VideoFileCube`` of the fit: the frames of ``frame_range`` of the file, or ``frames`` at ``coded_size`` in their place (what
    ``prepare_source`` returned).  An ``rgb24`` source with weights or ``film_grain`` is a ``ValueError`` here, before the fit starts."""
    from .frames_in import VideoFileCube
    cube = VideoFileCube(video, optical_flow_dir=options.flow_dir, W=options.video_size[0], H=options.video_size[1],
                         fmt=options.video_format, device=device, frame_range=frame_range, frames=frames, frame_size=coded_size)
    if options.weighted and cube.fmt.layout == "rgb24":
        raise ValueError("encode_gop: the weighted PSNR of a weighted fit is taken on luma codes; an rgb24 source has none")
    if options.film_grain and cube.fmt.layout == "rgb24":
        raise ValueError("encode_gop: film grain is measured and synthesised in the delivered Y'CbCr domain; an rgb24 source has none")
    return cube


def fit_gop(cube, device, options, display_size=None, denoise_log=None):
    """The fit and the stream encode -> ``(image, log, weights)``.  The flow of the cube (estimated on its frames, of ``flow_dir``, or
    none: ``optical_lambda = 0``) -> ``configure_fit`` and ``new_fit`` -> ``steps`` steps -> ``conduct_stream_encoding`` with 8-bit MLPs ->
    ``bitstream_bytes``: the file image, still without picture hashes.  ``weights``: None, or for a weighted fit (what a log says of the
    maps, the maps on the host); they are built on the cube's frames, the rectangles of ``roi`` scaled from ``display_size`` to them.
    Log entries: "W", "H", "frames", "steps", ("denoise": ``denoise_log``), "init", ("init_cell", "init_mix": with init="detail" only),
    "anchors_initial": the anchors after the voxel merge of ``create_from_points``, "loss_domain", "loss_matrix", "distortion",
    "fit_seconds", "anchors_coded"."""
    import os
    import tempfile
    import time

    from .arguments import cfg_20240919
    from .bitstream import CubeGeometry, bitstream_bytes
    from .stream_codec import conduct_stream_encoding
    o, geometry_source = options, cube
    mp_, opt, pipe = cfg_20240919()
    log = {"W": cube.width, "H": cube.height, "frames": cube.len_z_frames, "steps": int(o.steps)}
    if denoise_log is not None:
        log["denoise"] = denoise_log
    if o.estimate_flow:
        from .flow import EstimatedFlowCube
        cube = EstimatedFlowCube(cube, device=device)
    elif o.flow_dir is None:
        opt.optical_lambda = 0.0
    configure_fit(mp_, opt, cube, o.steps, o.lmbda, o.slab_frames, o.densify_grad_threshold)
    opt.loss_domain, opt.distortion = o.loss_domain, o.distortion
    pc, trainer = new_fit(cube, mp_, opt, pipe, o.anchors, device,
                          **o.new_fit_keywords(roi_base_hw=display_size and (display_size[1], display_size[0])))
    weights = (trainer.weighting, trainer.weight_maps.cpu()) if o.weighted else None
    log.update(o.init_log(), anchors_initial=int(pc._anchor.shape[0]), loss_domain=trainer.loss_domain, loss_matrix=trainer.loss_matrix,
               distortion=trainer.distortion)
    bg = trainer.background
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(1, int(o.steps) + 1):
        trainer.step(it)
    torch.cuda.synchronize()
    log["fit_seconds"] = time.perf_counter() - t0
    trainer.sync_replicas()
    trainer.close()
    with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
        mlp_file = os.path.join(tmp, "mlp.bin")
        pack = conduct_stream_encoding(pc, mlp_file=mlp_file)          # (quantises the MLPs of pc in place: the shipped form)
        with open(mlp_file, "rb") as f:
            mlp_bytes = f.read()
    log["anchors_coded"] = int(pack.n)
    return bitstream_bytes(pc, pack, CubeGeometry.of(geometry_source, mp_, pipe, bg.tolist()), mlp_bytes), log, weights


def verify_decode(image, device, options):
    """The decoder's own path on the file image -> ``(the image with the section PHSH, log entries)``: it is decoded into a null sink by
    the function, batch size and format the decoder will use (``decode_video``), and the hashes are those of the pictures IT produces.
    Log entries: "hash_format", "verify_decode_fps"."""
    from .bitstream import NullSink, decode_video, parse_bitstream, with_hashes
    from .frames_out import FrameFormat
    fmt = options.hash_format or FrameFormat("yuv420p")
    res = decode_video(parse_bitstream(image), NullSink(), fmt=fmt, verify=True, device=device)
    return with_hashes(image, fmt, res["hashes"]), {"hash_format": fmt.name, "verify_decode_fps": res["fps"]}


def measure_weighting(image, device, options, fmt, source, weights, fit_frames=None):
    """A weighted fit (else nothing happens): the weights only shaped the fit, so the image stays as it is.  It is decoded once more,
    into the format and size of the frames the fit saw (``fit_frames``; None: those of ``source = (video, frame_range)``).
    Log entry: "weighting": {"sources", "cell", ("strength", "clamp": activity), ("roi": the scaled rectangles), "min", "max", "psnr_y",
    "wpsnr_y": ``coded_wpsnr``}."""
    from .bitstream import parse_bitstream
    if weights is None:
        return image, {}
    if fit_frames is None:
        fit_frames = source_range(*source, options)[1]
    psnr_y, wpsnr_y = coded_wpsnr(parse_bitstream(image), fit_frames, fmt, weights[1], weights[0]["cell"], device)
    return image, {"weighting": dict(weights[0], psnr_y=psnr_y, wpsnr_y=wpsnr_y)}


def measure_display(image, device, options, fmt, source, display_size):
    """``coded_size`` (else nothing happens): the image gets the section DISP (the source's size and the filter) and is decoded once
    more, into the source's format at display size, against the ORIGINAL source's codes (``display_psnr``).
    Log entry: "display": {"W", "H", "filter": "lanczos3", "psnr_y", "psnr_611": (6 Y + U + V) / 8 of the plane PSNRs}."""
    from .bitstream import parse_bitstream, with_display
    if display_size is None:
        return image, {}
    image = with_display(image, display_size)
    psnr_y, psnr_611 = display_psnr(parse_bitstream(image), source_range(*source, options)[1], fmt, device)
    return image, {"display": {"W": display_size[0], "H": display_size[1], "filter": "lanczos3", "psnr_y": psnr_y, "psnr_611": psnr_611}}


def measure_grain(image, device, options, fmt, source):
    """``film_grain`` (else nothing happens): the image is decoded once more, into the SOURCE's own format, and the flat-block statistics
    of the ORIGINAL source's codes against it (``grain_statistics``; with ``denoise`` the grain the prefilter removed is what the decoder
    puts back) are fitted to film-grain parameters (``grain.fit_grain`` with ``grain_gain``; ``grain_seed`` None: a seed derived from the
    image as it stands here), which the image then carries as its section GRAN.  The picture hashes stay those of the ungrained pictures.
    Log entry: "grain": {"seed", "scale", "kx", "ky", "source", "blocks", "gain"}."""
    import hashlib

    from .bitstream import parse_bitstream, with_grain
    from .grain import blocks_used, fit_grain
    if not options.film_grain:
        return image, {}
    hdr, frames = source_range(*source, options)
    stats = grain_statistics(parse_bitstream(image), frames, int(hdr["H"]), int(hdr["W"]), fmt, device,
                             flat_threshold=options.grain_flat_threshold, max_residual=options.grain_max_residual)
    seed = int.from_bytes(hashlib.sha256(image).digest()[:8], "little") if options.grain_seed is None else int(options.grain_seed)
    params = fit_grain(stats, seed, gain=float(options.grain_gain), source=fmt)
    return with_grain(image, params), {"grain": dict(params.summary(), blocks=blocks_used(stats), gain=float(options.grain_gain))}


def encode_gop(video, device, frame_range=None, options=None, **fields):
    """One group of pictures of a video file -> ``(the bytes of a complete GSVC file, log)``: what tools/gsvc_encode.py does with a whole
    clip, for the frames ``frame_range = (first, stop)`` of it (None: all).  ``options``: an ``encode_options.EncodeOptions``, which
    documents every option, or its fields as keywords (both: ``TypeError``).  The stages and the log entries of each are in the
    docstrings of the functions this calls; the module's docstring has the table."""
    from .bitstream import unpack_sections
    from .encode_options import EncodeOptions
    if options is not None and fields:
        raise TypeError("encode_gop: give options= or its fields as keywords, not both")
    o, source = EncodeOptions(**fields) if options is None else options, (video, frame_range)
    frames, coded_size, display_size, denoise_log = prepare_source(video, device, frame_range, o)
    cube = source_cube(video, device, frame_range, o, frames, coded_size)
    frames, fmt = frames if o.weighted else None, cube.fmt          # (a weighted fit keeps what it saw on the host, for its weighted PSNR)
    image, log, weights = fit_gop(cube, device, o, display_size, denoise_log)
    del cube
    for stage, more in ((verify_decode, ()), (measure_weighting, (fmt, source, weights, frames)),
                        (measure_display, (fmt, source, display_size)), (measure_grain, (fmt, source))):
        release()
        image, entry = stage(image, device, o, *more)
        log.update(entry)
    release()
    log["sections"] = {t.decode("ascii"): len(p) for t, p in unpack_sections(image)}
    return image, log


