#!/usr/bin/env python3
"""Measurements of the spatially weighted distortion -> profiles/wdist.json.  Needs the GPU.

    python tools/bench_wdist.py kernels            weighted against unweighted SSIM + L1 pair kernels at 1080p, and block_sse against plane_sse
    python tools/bench_wdist.py step               bench.py's 1080p fitting step with all-ones maps against the same step without maps
    python tools/bench_wdist.py fits [--steps N]   deterministic fits of the 1080p synthetic clip: default, --weighting activity, a central ROI
    ... --json PATH                                where the section is merged into (default profiles/wdist.json)

Every comparison runs both sides in ONE process and alternates them in blocks (the host is shared: a difference is read against the spread
of the blocks, which is recorded).  Times are device events around blocks of calls; nothing is traced while timing."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed_blocks(torch, sides, blocks, reps):
    """{name: [ms per call of each block]} for callables ``sides = {name: fn}``, alternated block by block, device events."""
    out = {k: [] for k in sides}
    for fn in sides.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(blocks):
        for name, fn in sides.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                fn()
            t1.record()
            t1.synchronize()
            out[name].append(t0.elapsed_time(t1) / reps)
    return out


def _summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "blocks": len(ms)}


def run_kernels(args):
    import torch

    from gsvc_amd import metrics, wdist
    from gsvc_amd.detail import map_shape
    from gsvc_amd.frames_out import FrameFormat, frame_bytes
    from gsvc_amd.loss_utils import ssim_l1, wssim_l1
    H, W, cell = 1080, 1920, 8
    g = torch.Generator(device="cuda").manual_seed(0)
    f = torch.rand(3, H, W, device="cuda", generator=g, requires_grad=True)
    b = torch.rand(3, H, W, device="cuda", generator=g, requires_grad=True)
    gt = torch.rand(3, H, W, device="cuda", generator=g)
    wts = 0.25 + 3.75 * torch.rand(map_shape(H, W, cell), device="cuda", generator=g)

    def plain():
        s, l, _ = ssim_l1(f, gt, img_b=b)
        torch.autograd.grad(s + l, (f, b))

    def weighted():
        s, l, _ = wssim_l1(f, gt, wts, cell, img_b=b)
        torch.autograd.grad(s + l, (f, b))

    t = _timed_blocks(torch, {"ssim_l1_pair": plain, "wssim_l1_pair": weighted}, args.blocks, args.reps)
    res = {"shape": [3, H, W], "cell": cell, "what": "pair forward + backward per 1080p three-channel picture, autograd wrappers included",
           "ssim_l1_pair": _summary(t["ssim_l1_pair"]), "wssim_l1_pair": _summary(t["wssim_l1_pair"])}
    res["ratio_weighted_over_plain"] = res["wssim_l1_pair"]["median_ms"] / res["ssim_l1_pair"]["median_ms"]
    fmt = FrameFormat("yuv420p")
    n, nbytes = 16, frame_bytes(H, W, fmt)
    a8 = torch.randint(0, 256, (n, nbytes), device="cuda", dtype=torch.uint8, generator=g)
    b8 = torch.randint(0, 256, (n, nbytes), device="cuda", dtype=torch.uint8, generator=g)
    assert torch.equal(wdist.block_sse(a8, b8, H, W, fmt, cell).sum(dim=(1, 2)), metrics.plane_sse(a8, b8, H, W, fmt)[:, 0])
    t = _timed_blocks(torch, {"plane_sse": lambda: metrics.plane_sse(a8, b8, H, W, fmt),
                              "block_sse": lambda: wdist.block_sse(a8, b8, H, W, fmt, cell)}, args.blocks, args.reps)
    sse = {"frames": n, "format": fmt.name, "cell": cell, "what": "16 frames of 1080p per call; plane_sse reads all three planes, block_sse the luma",
           "plane_sse": _summary(t["plane_sse"]), "block_sse": _summary(t["block_sse"])}
    sse["ratio_block_over_plane"] = sse["block_sse"]["median_ms"] / sse["plane_sse"]["median_ms"]
    return {"kernels": res, "block_sse": sse}


def run_step(args):
    import torch

    import bench
    from gsvc_amd.detail import map_shape
    from gsvc_amd.loss_utils import StepDistortion
    from gsvc_amd.train import Trainer
    dev = torch.device("cuda", 0)
    bargs = SimpleNamespace(cfg3=False, anchors=245_000, train_frames=64, height=1080, width=1920, scene_seed=0)
    cube, mp_, opt, pipe, pc, _ = bench.headline_model(bargs, dev)
    trainer = Trainer(pc, cube, opt, pipe, mp_, seed=0)
    cell = 8
    ones = torch.ones((64,) + map_shape(1080, 1920, cell), device=dev)
    plain, weighted = trainer._distortion, StepDistortion(opt, cube, weight_maps=ones, weight_cell=cell)
    it = [0]

    def step_with(dist):
        def step():
            trainer._distortion = dist
            it[0] += 1
            trainer.step(it[0], frame_idx=it[0] % 60)
        return step

    for _ in range(args.pretrain):
        step_with(plain)()
    t = _timed_blocks(torch, {"plain": step_with(plain), "all_ones_maps": step_with(weighted)}, args.blocks, args.reps)
    trainer.close()
    res = {"what": "bench.py's configs[2] fitting step (1080p, 245 000 anchors, entropy-constrained phase), the same trainer, the distortion "
                   "object swapped block by block; 'plain' launches exactly what the step launched before this feature",
           "pretrain_steps": args.pretrain, "plain": _summary(t["plain"]), "all_ones_maps": _summary(t["all_ones_maps"])}
    res["ratio_weighted_over_plain"] = res["all_ones_maps"]["median_ms"] / res["plain"]["median_ms"]
    return {"step": res}


def run_fits(args):
    import copy
    import tempfile

    import numpy as np
    import torch

    from gsvc_amd import switches, wdist
    from gsvc_amd.arguments import cfg_20240919
    from gsvc_amd.detail import cube_detail
    from gsvc_amd.fit_setup import configure_fit, new_fit
    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import FrameFormat, frames_to_u8
    from gsvc_amd.ortho_gaussian_renderer import render_frames
    from gsvc_amd.report import evaluate
    from gsvc_amd.stream_codec import conduct_stream_decoding, conduct_stream_encoding
    os.environ["GSVC_DETERMINISTIC"] = "1"
    switches.reload()
    dev = torch.device("cuda", 0)
    H, W, T, cell = 1080, 1920, 64, 8
    fmt = FrameFormat("yuv420p")
    roi = (W // 4, H // 4, W // 2, H // 2, 4.0)          # central, cell-aligned at 8: 480, 270 -> rows 270 .. 810 are not: report on cells wholly inside
    cube = SyntheticFrameCube(H, W, T, seed=1234, device=dev).materialize()
    activity = wdist.activity_weights(cube_detail(cube, cell), H, W, cell, 16)
    inside = wdist._roi64(H, W, cell, [roi[:4] + (2.0,)], 1)[0] == 2.0          # the cells wholly inside the rectangle
    eval_ids = [int(round(i)) for i in np.linspace(0, T - 1, 16)]
    configs = {"default": {}, "activity": dict(weighting="activity", weight_cell=cell), "roi": dict(roi=[roi], weight_cell=cell)}
    rows = {}
    for name, kw in configs.items():
        if args.only and name not in args.only:
            continue
        mp_, opt, pipe = cfg_20240919()
        configure_fit(mp_, opt, cube, args.steps, 0.004, 16.0, None)
        pc, trainer = new_fit(cube, mp_, opt, pipe, 100_000, dev, **kw)
        bg = trainer.background
        for it in range(1, args.steps + 1):
            trainer.step(it)
        torch.cuda.synchronize()
        trainer.sync_replicas()
        trainer.close()
        with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
            q = copy.deepcopy(pc)
            mlp_file = os.path.join(tmp, "mlp.bin")
            pack = conduct_stream_encoding(q, mlp_file=mlp_file)
            pack.save(os.path.join(tmp, "streams"))
            total = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(tmp) for f in fs)
            dec = conduct_stream_decoding(copy.deepcopy(q), pack, mlp_file=mlp_file)
            ev = evaluate(dec, cube, pipe, bg, frame_ids=eval_ids, delivered=fmt, code_metrics=True, weight_maps=activity, weight_cell=cell)
            frames = [cube[i] for i in eval_ids]
            rendered = [torch.clamp(img, 0, 1) for img in render_frames(frames, dec, pipe, bg, batch=8)]
            src = frames_to_u8([torch.clamp(fr.image.to(dev), 0, 1).permute(0, 2, 1).contiguous() for fr in frames], fmt)
            sse = wdist.block_sse(frames_to_u8(rendered, fmt), src, H, W, fmt, cell).cpu().numpy().astype(np.float64)
        px = wdist.cell_pixels(H, W, cell)
        psnr = lambda m: 10.0 * float(np.log10(255.0 ** 2 * len(eval_ids) * px[m].sum() / sse[:, m].sum()))       # noqa: E731
        rows[name] = {"bpp": 8.0 * total / (H * W * T), "psnr_y": ev["psnr_y"], "wpsnr_y_activity_maps": ev["wpsnr_y"], "psnr_611": ev["psnr_611"],
                      "msssim_y": ev["msssim_y"], "psnr_y_inside_roi": psnr(inside), "psnr_y_outside_roi": psnr(~inside),
                      "anchors_coded": int(pack.n)}
        print(name, json.dumps(rows[name]), flush=True)
        _merge(args.json, {"fits": {"rows": dict(rows)}})          # kept fit by fit: a run that is cut short leaves what it finished
        del pc, trainer, dec, q, pack
        torch.cuda.empty_cache()
    return {"fits": {"what": f"one deterministic {args.steps}-step fit each of the 1080p synthetic clip (64 frames, 100 000 initial anchors, one seed), "
                             "the 8-bit-MLP decoded model evaluated on 16 frames as yuv420p codes; wPSNR-Y under the activity maps for every fit; "
                             "inside / outside: the cells wholly inside the ROI rectangle against the rest",
                     "roi": list(roi), "cell": cell, "activity_strength": wdist.DEFAULT_STRENGTH, "rows": rows}}


def _merge(path, res):
    """``res`` into the JSON file at ``path``, section by section; the rows of "fits" are merged, not replaced."""
    old = {}
    if os.path.exists(path):
        with open(path) as f:
            old = json.load(f)
    if "fits" in res and "fits" in old:
        rows = dict(old["fits"].get("rows", {}), **res["fits"].get("rows", {}))
        res = dict(res, fits=dict(dict(old["fits"], **res["fits"]), rows=rows))
    old.update(res)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(old, f, indent=1)
        f.write("\n")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernels", "step", "fits"))
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pretrain", type=int, default=60)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "wdist.json"))
    args = ap.parse_args(argv)
    res = {"kernels": run_kernels, "step": run_step, "fits": run_fits}[args.what](args)
    _merge(args.json, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
