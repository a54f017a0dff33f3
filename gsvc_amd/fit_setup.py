"""The set-up of a fit that tools/fit_synthetic.py and tools/gsvc_encode.py share: the reference's 40 000-iteration schedule scaled to
a run's length, the model, its initial anchors and the Trainer on a frame cube, and ``encode_gop``: a range of frames of a video file
fitted, stream-encoded and verified into the bytes of one bitstream file (a whole clip, or one group of pictures of a sequence file).

The reference's schedule (pipeline/train.py:325-583: 10 k full precision / 5 k quantised / 20 k entropy-constrained / 5 k
straight-through; statistics from 500, densification 1 500 .. 25 000 every 100, paused 1 000 iterations at the first phase change) is
scaled to ``steps`` iterations with the same proportions.
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
    if maps is None:
        trainer = Trainer(pc, cube, opt, pipe, mp_, seed=0)
    else:
        trainer = Trainer(pc, cube, opt, pipe, mp_, seed=0, weight_maps=maps, weight_cell=weighting_info["cell"])
    trainer.weighting = weighting_info
    return pc, trainer


def grain_statistics(bs, source_frames, H: int, W: int, fmt, device, batch: int = 8, flat_threshold=None, max_residual=None):
    """The film-grain statistics of a file image against its source: ``bs`` (a parsed ``Bitstream``) is decoded into ``fmt``, the SOURCE's
    own format, batch by batch, each batch's ``grain.grain_stats`` against the source's codes (``source_frames``: the host array
    ``[T, frame_bytes]`` of ``frames_in.open_video``, uploaded a batch at a time) is taken on the device, and the batches are summed on
    the host as Python ints -> nested lists ``[3][16][6]``.  ``flat_threshold``, ``max_residual``: the two rejection thresholds of
    ``grain.grain_stats`` (None: its defaults, which are starting values)."""
    from .frames_out import render_frames_u8
    from .grain import BINS, DEFAULT_FLAT_THRESHOLD, DEFAULT_MAX_RESIDUAL, grain_stats
    flat = DEFAULT_FLAT_THRESHOLD if flat_threshold is None else int(flat_threshold)
    worst = DEFAULT_MAX_RESIDUAL if max_residual is None else int(max_residual)
    total = [[[0] * 6 for _ in range(BINS)] for _ in range(3)]
    pc, cams, pipe, bg = bs.build_model(device)
    at = [0]

    def take(rows):
        n = int(rows.shape[0])
        src = torch.from_numpy(np.ascontiguousarray(source_frames[at[0]:at[0] + n])).to(rows.device)
        part = grain_stats(src, rows, H, W, fmt, flat_threshold=flat, max_residual=worst).cpu().tolist()
        for p in range(3):
            for b in range(BINS):
                for j in range(6):
                    total[p][b][j] += int(part[p][b][j])
        at[0] += n

    with torch.no_grad():
        for _ in render_frames_u8(cams, pc, pipe, bg, fmt=fmt, batch=int(batch), to_host=False, on_device_batch=take):
            pass
    if at[0] != int(source_frames.shape[0]):
        raise ValueError(f"grain_statistics: the file decodes to {at[0]} frames, the source has {int(source_frames.shape[0])}")
    return total


def display_psnr(bs, source_frames, fmt, device, batch: int = 8):
    """What a reduced-resolution file delivers against its source: ``bs`` (a parsed ``Bitstream`` with a DISP section) is decoded into
    ``fmt``, the SOURCE's own format, at display size, batch by batch, and each batch's ``metrics.plane_sse`` against the source's codes
    (``source_frames``: the host array ``[T, frame_bytes]`` at display size, uploaded a batch at a time) is summed over all frames ->
    ``(psnr_y, psnr_611)``, the latter ``(6 Y + U + V) / 8`` of the three plane PSNRs."""
    from .frames_out import render_frames_u8
    from .metrics import plane_samples, plane_sse, psnr_of_sse
    W, H = bs.display_size
    cW, cH = bs.coded_size
    pc, cams, pipe, bg = bs.build_model(device)
    total = torch.zeros(3, dtype=torch.int64, device=device)
    got, rows = 0, []
    with torch.no_grad():
        for row in render_frames_u8(cams, pc, pipe, bg, fmt=fmt, batch=int(batch), to_host=False,
                                    out_size=None if (W, H) == (cW, cH) else (H, W)):
            rows.append(row)
            if len(rows) == int(batch) or got + len(rows) == len(cams):
                src = torch.from_numpy(np.ascontiguousarray(source_frames[got:got + len(rows)])).to(row.device)
                total += plane_sse(torch.stack(rows), src, H, W, fmt).sum(dim=0)
                got += len(rows)
                rows = []
    if got != int(source_frames.shape[0]):
        raise ValueError(f"display_psnr: the file decodes to {got} frames, the source has {int(source_frames.shape[0])}")
    peak = float((1 << fmt.depth) - 1)
    samples = torch.tensor(plane_samples(H, W, fmt), dtype=torch.float64, device=total.device) * got
    p = [float(v) for v in psnr_of_sse(total, samples, peak).tolist()]
    return p[0], (6.0 * p[0] + p[1] + p[2]) / 8.0


def coded_wpsnr(bs, fit_frames, fmt, weight_maps, cell: int, device, batch: int = 8):
    """What a weighted fit bought, on the delivered codes: ``bs`` (a parsed ``Bitstream``) is decoded into ``fmt``, the format of the frames
    the fit was given, at the size it was fitted at, batch by batch, and each batch's ``wdist.block_sse`` against those frames
    (``fit_frames``: the host array ``[T, frame_bytes]``, uploaded a batch at a time) is kept -> ``(psnr_y, wpsnr_y)`` pooled over the
    frames: the plain luma PSNR and ``wdist.weighted_psnr_y`` under ``weight_maps`` ``[T, Hc, Wc]``."""
    from .frames_out import render_frames_u8
    from .wdist import block_sse, weighted_psnr_y
    W, H = bs.coded_size
    pc, cams, pipe, bg = bs.build_model(device)
    blocks, rows, got = [], [], 0
    with torch.no_grad():
        for row in render_frames_u8(cams, pc, pipe, bg, fmt=fmt, batch=int(batch), to_host=False):
            rows.append(row)
            if len(rows) == int(batch) or got + len(rows) == len(cams):
                src = torch.from_numpy(np.ascontiguousarray(fit_frames[got:got + len(rows)])).to(row.device)
                blocks.append(block_sse(torch.stack(rows), src, H, W, fmt, cell).cpu())
                got += len(rows)
                rows = []
    if got != int(fit_frames.shape[0]):
        raise ValueError(f"coded_wpsnr: the file decodes to {got} frames, the fit saw {int(fit_frames.shape[0])}")
    sse = torch.cat(blocks)
    _, plain = weighted_psnr_y(sse, torch.ones(sse.shape, dtype=torch.float64), fmt.depth, H, W)
    _, weighted = weighted_psnr_y(sse, weight_maps, fmt.depth, H, W)
    return plain, weighted


def encode_gop(video, device, frame_range=None, steps: int = 2000, lmbda: float = 0.004, anchors: int = 100_000, slab_frames: float = 16.0,
               densify_grad_threshold=None, estimate_flow: bool = False, flow_dir=None, video_size=(None, None), video_format=None,
               hash_format=None, loss_domain: str = "rgb", init: str = "uniform", init_cell: int = 8, init_mix: float = 0.25,
               distortion: str = "ssim", film_grain: bool = False, grain_gain: float = 1.0, grain_seed=None,
               grain_flat_threshold=None, grain_max_residual=None, denoise=None, denoise_gain: float = 1.0, coded_size=None,
               weighting=None, weight_strength: float = 0.5, weight_cell=None, roi=None, weight_file=None):
    """One group of pictures of a video file -> ``(the bytes of a complete GSVC file, log)``: what tools/gsvc_encode.py does with a whole
    clip, for the frames ``frame_range = (first, stop)`` of it (None: all).  VideoFileCube (optionally with the flow estimated from the
    frames) -> the fit -> ``conduct_stream_encoding`` with 8-bit MLPs -> the file image; that image is then decoded into a null sink by
    the function, batch size and format the decoder will use (``decode_video``), which yields the picture hashes it is given as its PHSH
    section.  The trainer, the cube and the model are released before this returns.  ``loss_domain``: where the fit takes its
    distortion (``OptimizationParams.loss_domain``; the bitstream and the decoder are the same for every domain); ``distortion``: its
    structural term, "ssim" or "ms_ssim" (``OptimizationParams.distortion``).  ``film_grain``: after the verification decode the file
    image is decoded once more, into the SOURCE's own format, and the flat-block statistics of the source's codes against it
    (``grain_statistics``) are fitted to film-grain parameters (``grain.fit_grain`` with ``grain_gain``; ``grain_seed`` None: a seed
    derived from the file image; ``grain_flat_threshold``, ``grain_max_residual`` None: the defaults of ``grain.grain_stats``), which the
    file carries as its GRAN section; the picture hashes stay those of the ungrained
    pictures, and an ``rgb24`` source is a ``ValueError`` before the fit starts.  The log then has "grain": {"seed", "scale", "kx", "ky",
    "source", "blocks", "gain"}.  ``denoise``: None (the default: the source as it is), "auto" or a noise sigma in codes: the frames of
    ``frame_range`` are first put through the motion-compensated temporal prefilter (``tfilter.denoise_frames`` with ``denoise_gain``; one
    GOP, so nothing is filtered across its ends) and the fit is given the filtered frames; an ``rgb24`` source is a ``ValueError``.  The log
    then has "denoise": {"sigma", "q", "source", "gain", "psnr_y"}.  With ``film_grain`` as well the grain statistics stay measured
    against the ORIGINAL source (``video`` is reopened for them), so the grain the prefilter removed is what the decoder puts back.
    ``coded_size=(Wc, Hc)`` (None: the source's size): reduced-resolution coding (gsvc_amd/resample.py).  The frames of ``frame_range``
    — with ``denoise`` the filtered ones, filtered at source size — are resampled on the device, in chunks of 16, to ``Wc x Hc`` in the
    source's own format, and the fit is given the resampled frames (``estimate_flow`` estimates on them); HEAD carries the coded size,
    the section DISP the source's size and the filter, PHSH the hashes of the coded-size pictures.  The file image is then decoded
    once more, into the source's format at display size, and compared with the ORIGINAL source's codes (``metrics.plane_sse`` over all
    frames): "W" / "H" of the log are the coded size and the log has "display": {"W", "H", "filter": "lanczos3", "psnr_y", "psnr_611":
    (6 Y + U + V) / 8 of the plane PSNRs}.  A ``ValueError`` before anything is fitted: ``flow_dir`` (those flows are at source size) or
    ``film_grain`` with ``coded_size``, an ``rgb24`` source, a ratio above 4, an odd size for 4:2:0.  ``init``,
    ``init_cell``, ``init_mix``: where the fit's first anchors come from (``new_fit``; anchors are coded wherever they are).  ``log``:
    {"W", "H", "frames", "steps", "init", ("init_cell", "init_mix": with init="detail" only), "anchors_initial": the anchors after the
    voxel merge of ``create_from_points``, "loss_domain", "loss_matrix", "distortion", "anchors_coded", "fit_seconds", "hash_format",
    "verify_decode_fps", "sections"}.  ``weighting="activity"`` (with ``weight_strength``), ``roi=[(x, y, w, h, weight), ...]`` in the
    SOURCE's pixels, ``weight_file`` (a ``.npy``), all at cells of ``weight_cell`` pixels (None: 8): spatially weighted distortion
    (``new_fit``, gsvc_amd/wdist.py).  The maps are built on the frames the fit sees — of this ``frame_range`` alone, filtered and at
    coded size where those are asked for, rectangles scaled to it — and only shape the fit: the file's sections are what they were.  The
    file image is then decoded once more, into the format and size of those frames, and the log has "weighting": {"sources", "cell",
    ("strength", "clamp": activity), ("roi": the scaled rectangles), "min", "max", "psnr_y", "wpsnr_y": ``coded_wpsnr``}; an ``rgb24``
    source is a ``ValueError`` before the fit starts.  Without these arguments the log has no such entry."""
    import gc
    import os
    import tempfile
    import time

    from .arguments import cfg_20240919
    from .bitstream import CubeGeometry, NullSink, bitstream_bytes, decode_video, parse_bitstream, unpack_sections, with_hashes
    from .frames_in import VideoFileCube
    from .frames_out import FrameFormat
    from .stream_codec import conduct_stream_encoding
    mp_, opt, pipe = cfg_20240919()
    filtered, denoise_log, frame_size = None, None, None
    weighted = weighting is not None or bool(roi) or weight_file is not None
    if coded_size is not None:
        try:
            frame_size = tuple(int(v) for v in coded_size)
        except (TypeError, ValueError):
            frame_size = ()
        if len(frame_size) != 2:
            raise ValueError(f"encode_gop: coded_size must be (W, H) (got {coded_size!r})")
        if flow_dir is not None:
            raise ValueError("encode_gop: the flows of flow_dir are at the source's size; with coded_size use estimate_flow")
        if film_grain:
            raise ValueError("encode_gop: film_grain with coded_size is not supported (the grain would be measured at one size and "
                             "synthesised at another)")
    if denoise is not None or frame_size is not None:
        from .frames_in import open_video
        hdr, source = open_video(video, video_size[0], video_size[1], video_format)
        if hdr["fmt"].layout == "rgb24":
            raise ValueError("encode_gop: the temporal prefilter and the resampler work on Y'CbCr codes; an rgb24 source has none")
        if frame_size is not None:
            from .resample import check_sizes
            check_sizes(int(hdr["H"]), int(hdr["W"]), frame_size[1], frame_size[0], hdr["fmt"], "encode_gop: coded_size")
        if frame_range is not None:
            try:
                first, stop = (int(v) for v in frame_range)
            except (TypeError, ValueError):
                raise ValueError(f"encode_gop: frame_range must be (first, stop) (got {frame_range!r})") from None
            if not 0 <= first < stop <= int(source.shape[0]):          # (what VideoFileCube refuses, before anything is filtered)
                raise ValueError(f"encode_gop: frame_range ({first}, {stop}) is not a non-empty range inside the {int(source.shape[0])} "
                                 f"frames of {video}")
            source = source[first:stop]
        if denoise is not None:
            from .tfilter import denoise_range
            filtered, denoise_log = denoise_range(source, int(hdr["H"]), int(hdr["W"]), hdr["fmt"], device, sigma=denoise,
                                                  gain=float(denoise_gain))
        if frame_size is not None:
            from .resample import resample_range
            filtered = resample_range(source if filtered is None else filtered, int(hdr["H"]), int(hdr["W"]), hdr["fmt"], frame_size[1],
                                      frame_size[0], device)
            display = (int(hdr["W"]), int(hdr["H"]))
        del source
    cube = VideoFileCube(video, optical_flow_dir=flow_dir, W=video_size[0], H=video_size[1], fmt=video_format, device=device,
                         frame_range=frame_range, frames=filtered, frame_size=frame_size)
    fit_frames = filtered if weighted else None          # what the fit sees, for the weighted PSNR of the file image
    del filtered
    if weighted and cube.fmt.layout == "rgb24":
        raise ValueError("encode_gop: the weighted PSNR of a weighted fit is taken on luma codes; an rgb24 source has none")
    if film_grain and cube.fmt.layout == "rgb24":
        raise ValueError("encode_gop: film grain is measured and synthesised in the delivered Y'CbCr domain; an rgb24 source has none")
    source_fmt = cube.fmt
    log = {"W": cube.width, "H": cube.height, "frames": cube.len_z_frames, "steps": int(steps)}
    if denoise_log is not None:
        log["denoise"] = denoise_log
    geometry_source = cube
    if estimate_flow:
        from .flow import EstimatedFlowCube
        cube = EstimatedFlowCube(cube, device=device)
    elif flow_dir is None:
        opt.optical_lambda = 0.0
    configure_fit(mp_, opt, cube, steps, lmbda, slab_frames, densify_grad_threshold)
    opt.loss_domain = loss_domain
    opt.distortion = distortion
    if weighted:
        pc, trainer = new_fit(cube, mp_, opt, pipe, anchors, device, init=init, init_cell=init_cell, init_mix=init_mix, weighting=weighting,
                              weight_strength=weight_strength, weight_cell=weight_cell, roi=roi, weight_file=weight_file,
                              roi_base_hw=(display[1], display[0]) if frame_size is not None else None)
        weighting_log, weight_maps = trainer.weighting, trainer.weight_maps.cpu()
    else:
        pc, trainer = new_fit(cube, mp_, opt, pipe, anchors, device, init=init, init_cell=init_cell, init_mix=init_mix)
    log["init"] = init
    if init == "detail":
        log["init_cell"], log["init_mix"] = int(init_cell), float(init_mix)
    log["anchors_initial"] = int(pc._anchor.shape[0])
    log["loss_domain"], log["loss_matrix"] = trainer.loss_domain, trainer.loss_matrix
    log["distortion"] = trainer.distortion
    bg = trainer.background
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(1, int(steps) + 1):
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
    blob = bitstream_bytes(pc, pack, CubeGeometry.of(geometry_source, mp_, pipe, bg.tolist()), mlp_bytes)
    log["anchors_coded"] = int(pack.n)
    # the decoder's own path on the file image: the hashes are those of the pictures IT produces
    del trainer, cube, geometry_source, pc, pack
    gc.collect()
    fmt = hash_format or FrameFormat("yuv420p")
    res = decode_video(parse_bitstream(blob), NullSink(), fmt=fmt, verify=True, device=device)
    blob = with_hashes(blob, fmt, res["hashes"])
    del res["hashes"]
    gc.collect()
    torch.cuda.empty_cache()
    log["hash_format"], log["verify_decode_fps"] = fmt.name, res["fps"]
    if weighted:
        if fit_frames is None:
            from .frames_in import open_video
            _, fit_frames = open_video(video, video_size[0], video_size[1], video_format)
            if frame_range is not None:
                fit_frames = fit_frames[int(frame_range[0]):int(frame_range[1])]
        psnr_y, wpsnr_y = coded_wpsnr(parse_bitstream(blob), fit_frames, source_fmt, weight_maps, weighting_log["cell"], device)
        log["weighting"] = dict(weighting_log, psnr_y=psnr_y, wpsnr_y=wpsnr_y)
        del fit_frames
        gc.collect()
        torch.cuda.empty_cache()
    if frame_size is not None:
        from .bitstream import with_display
        from .frames_in import open_video
        blob = with_display(blob, display)
        _, source = open_video(video, video_size[0], video_size[1], video_format)
        if frame_range is not None:
            source = source[int(frame_range[0]):int(frame_range[1])]
        psnr_y, psnr_611 = display_psnr(parse_bitstream(blob), source, source_fmt, device)
        log["display"] = {"W": display[0], "H": display[1], "filter": "lanczos3", "psnr_y": psnr_y, "psnr_611": psnr_611}
        del source
        gc.collect()
        torch.cuda.empty_cache()
    if film_grain:
        import hashlib

        from .bitstream import with_grain
        from .frames_in import open_video
        from .grain import blocks_used, fit_grain
        _, source = open_video(video, video_size[0], video_size[1], video_format)
        if frame_range is not None:
            source = source[int(frame_range[0]):int(frame_range[1])]
        stats = grain_statistics(parse_bitstream(blob), source, log["H"], log["W"], source_fmt, device, flat_threshold=grain_flat_threshold,
                                 max_residual=grain_max_residual)
        seed = int.from_bytes(hashlib.sha256(blob).digest()[:8], "little") if grain_seed is None else int(grain_seed)
        params = fit_grain(stats, seed, gain=float(grain_gain), source=source_fmt)
        blob = with_grain(blob, params)
        log["grain"] = dict(params.summary(), blocks=blocks_used(stats), gain=float(grain_gain))
        del source
        gc.collect()
        torch.cuda.empty_cache()
    log["sections"] = {t.decode("ascii"): len(p) for t, p in unpack_sections(blob)}
    return blob, log
