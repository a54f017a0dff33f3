#!/usr/bin/env python3
"""What film grain costs (csrc/grain.hip, k_grain_apply and k_grain_stats).  One JSON line.

  kernel    1080 x 1920 buffers of n = 8 frames, yuv420p and yuv420p10le, of a synthetic video (``SyntheticFrameCube`` converted by
            ``frames_to_u8``).  ``grain.apply_grain`` (in place, so the buffers keep gathering grain: the work per call is the same)
            and ``grain.grain_stats`` (the buffers against a copy with grain), alternated in the same process with
              frames_to_u8   the conversion the decoder already runs per batch, on the float pictures of the same frames;
              torch          the same operations as tensor expressions (int64 arithmetic for the hash; unfolded 8 x 8 blocks and
                             ``index_add_`` for the statistics), checked equal to the kernels before anything is timed.
            Device-event time of groups of 20 calls (the tensor expressions: 2), median over >= 30 groups, per frame.  The inputs rotate
            through enough sets to exceed the 256 MiB Infinity Cache.
  loop      the decoder loop ``render_frames_u8(to_host=True)`` of the fitted headline model of tools/bench_frames_out.py with and
            without ``grain``, alternated, frames per second over the whole loop (host clock around a final synchronise).
  closed    one fit and a measurement, nothing about visual quality: the headline model is fitted to the clean synthetic clip; the
            "source" is that clip's codes with grain of known parameters; ``grain_stats`` (source, decoded) -> ``fit_grain`` -> grain on
            the decoded frames.  Reported per luma bin: the flat-block sigma (block-DC-removed, 8-bit codes) of source against decoded
            beside that of grained-decoded against decoded, and the blocks that counted.

    python tools/bench_grain.py [--groups 30] [--anchors 245000 --fit-steps 200 --frames 48] [--no-loop] [--json profiles/grain.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gsvc_amd import frames_out as fo  # noqa: E402
from gsvc_amd import grain as G  # noqa: E402
from gsvc_amd.frames_out import FrameFormat  # noqa: E402

CACHE = 300 << 20          # rotate through more than the 256 MiB last-level cache
H, W = 1080, 1920
PARAMS = dict(seed=0x5EED, scale=((900,) * 17, (600,) * 17, (600,) * 17), kx=(16, 8, 8), ky=(12, 8, 8))
_M64 = (1 << 64) - 1


def timed_group(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(launches):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / launches          # seconds per call


# ---- the tensor-expression forms ----------------------------------------------------------------------------------------------
def _i64(v: int) -> int:
    v &= _M64
    return v - (1 << 64) if v >= 1 << 63 else v


def _lsr(z, k):
    return (z >> k) & ((1 << (64 - k)) - 1)


def _mix(z):
    z = (z ^ _lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _i64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def _mix_int(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def torch_noise(seed, f, p, h, w, kx, ky, dev):
    """n of an h x w plane as tensor expressions (int64 wraps as uint64 does)."""
    gold = 0x9E3779B97F4A7C15
    key = _mix_int((seed + (3 * f + p + 1) * gold) & _M64)
    Y = torch.arange(0, h + 2, device=dev, dtype=torch.int64)[:, None]
    X = torch.arange(0, w + 2, device=dev, dtype=torch.int64)[None, :]
    hsh = _mix(((Y << 32) | (X >> 1)) * _i64(gold) + _i64(key))
    wd = torch.where((X & 1) == 1, _lsr(hsh, 32), hsh & 0xFFFFFFFF)
    g = (wd & 255) + ((wd >> 8) & 255) + ((wd >> 16) & 255) + ((wd >> 24) & 255) - 510
    t = kx * (g[:, :-2] + g[:, 2:]) + 64 * g[:, 1:-1]
    return (ky * (t[:-2] + t[2:]) + 64 * t[1:-1] + 2048) >> 12


def _planes(frames, fmt):
    """[n, frame_bytes] -> int64 (y [n, H, W], u, v [n, H / 2, W / 2]) copies."""
    n = frames.shape[0]
    codes = frames.to(torch.int64) if fmt.depth == 8 else frames.view(torch.int16).to(torch.int64) & 0xFFFF
    ch, cw = H // 2, W // 2
    return (codes[:, :H * W].reshape(n, H, W), codes[:, H * W:H * W + ch * cw].reshape(n, ch, cw), codes[:, H * W + ch * cw:].reshape(n, ch, cw))


def torch_apply(frames, fmt, p: G.GrainParams, first=0):
    """A grained copy of [n, frame_bytes] yuv420p frames, limited range, as tensor expressions."""
    n, dev, up, S = frames.shape[0], frames.device, 1 << (fmt.depth - 8), 24 - fmt.depth
    planes = _planes(frames, fmt)
    luma = planes[0]
    out = []
    for k, c in enumerate(planes):
        m = luma if k == 0 else (luma[:, 0::2, 0::2] + luma[:, 0::2, 1::2] + luma[:, 1::2, 0::2] + luma[:, 1::2, 1::2] + 2) >> 2
        l = torch.clamp(m >> (fmt.depth - 8), max=255)
        sc = torch.tensor(p.scale[k], dtype=torch.int64, device=dev)
        s = (sc[l >> 4] * (16 - (l & 15)) + sc[(l >> 4) + 1] * (l & 15) + 8) >> 4
        nn = torch.stack([torch_noise(p.seed, first + f, k, c.shape[1], c.shape[2], p.kx[k], p.ky[k], dev) for f in range(n)])
        grain = (nn * s + (1 << (S - 1))) >> S
        lo, hi = 16 * up, (235 if k == 0 else 240) * up
        out.append(torch.minimum(torch.maximum(c + grain, torch.clamp(c, max=lo)), torch.clamp(c, min=hi)).reshape(n, -1))
    codes = torch.cat(out, 1)
    return codes.to(torch.uint8) if fmt.depth == 8 else codes.to(torch.int16).view(torch.uint8)


def torch_stats(src, dec, fmt, flat=G.DEFAULT_FLAT_THRESHOLD, worst=G.DEFAULT_MAX_RESIDUAL):
    """int64 [3, 16, 6] of two [n, frame_bytes] yuv420p buffers as tensor expressions."""
    up = 1 << (fmt.depth - 8)
    ps, pd = _planes(src, fmt), _planes(dec, fmt)
    out = torch.zeros((3 * 16, 6), dtype=torch.int64, device=src.device)

    def blocks(a, side=8):          # [n, h, w] -> [n, h / side, w / side, side, side], whole blocks only
        n, h, w = a.shape
        return a[:, :h // side * side, :w // side * side].reshape(n, h // side, side, w // side, side).permute(0, 1, 3, 2, 4)
    for k in range(3):
        d, r = blocks(pd[k]), blocks(ps[k]) - blocks(pd[k])
        A = (d[..., :, 1:] - d[..., :, :-1]).abs().sum((-1, -2)) + (d[..., 1:, :] - d[..., :-1, :]).abs().sum((-1, -2))
        if k == 0:
            lum = d.sum((-1, -2)) >> 6
        else:
            lum = blocks(pd[0], 16).sum((-1, -2))[:, :d.shape[1], :d.shape[2]] >> 8
        b = torch.clamp(lum >> (fmt.depth - 8), max=255) >> 4
        keep = (A <= flat * up) & (r.abs().amax((-1, -2)) <= worst * up)
        S1 = r.sum((-1, -2))
        rows = torch.stack([torch.ones_like(S1), S1, (r * r).sum((-1, -2)), S1 * S1, (r[..., :, :-1] * r[..., :, 1:]).sum((-1, -2)),
                            (r[..., :-1, :] * r[..., 1:, :]).sum((-1, -2))], -1)
        out.index_add_(0, (16 * k + b)[keep], rows[keep])
    return out.reshape(3, 16, 6)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------
def bench_case(depth, n, groups, dev):
    from gsvc_amd.frame import SyntheticFrameCube
    fmt = FrameFormat("yuv420p", depth=depth)
    nb = fo.frame_bytes(H, W, fmt)
    sets = max(2, -(-CACHE // (n * nb)))
    cube = SyntheticFrameCube(H, W, n + 1, seed=3, device=dev)
    imgs = [cube._image(t) for t in range(n + 1)]
    clean = [fo.frames_to_u8(imgs[k % 2:k % 2 + n], fmt).contiguous() for k in range(sets)]
    p = G.GrainParams(source=fmt, **PARAMS)
    work = [c.clone() for c in clean]
    noisy = [G.apply_grain(c.clone(), H, W, fmt, p) for c in clean[:2]]
    out_u8 = torch.empty((n, nb), dtype=torch.uint8, device=dev)
    # the kernels are the tensor expressions, at the size that is timed
    equal_apply = bool(torch.equal(torch_apply(clean[0][:2], fmt, p), noisy[0][:2]))
    equal_stats = bool(torch.equal(torch_stats(noisy[0], clean[0], fmt), G.grain_stats(noisy[0], clean[0], H, W, fmt)))
    same = bool(torch.equal(G.grain_stats(noisy[0], clean[0], H, W, fmt), G.grain_stats(noisy[0], clean[0], H, W, fmt)))

    def apply(k):
        return G.apply_grain(work[k % sets], H, W, fmt, p, first_frame=k)

    def stats(k):
        return G.grain_stats(noisy[k % 2], clean[k % sets], H, W, fmt)

    def convert(k):
        return fo.frames_to_u8(imgs[k % 2:k % 2 + n], fmt, out=out_u8)

    def apply_expr(k):
        return torch_apply(clean[k % sets], fmt, p, first=k)

    def stats_expr(k):
        return torch_stats(noisy[k % 2], clean[k % sets], fmt)
    fast, slow = (apply, stats, convert), (apply_expr, stats_expr)
    for _ in range(3):
        for fn in fast:
            timed_group(fn, 20)
        for fn in slow:
            timed_group(fn, 2)
    t = {fn.__name__: [] for fn in fast + slow}
    for _ in range(groups):          # alternated
        for fn in fast:
            t[fn.__name__].append(timed_group(fn, 20))
        for fn in slow:
            t[fn.__name__].append(timed_group(fn, 2))
    med = {k: statistics.median(v) for k, v in t.items()}
    res = {"case": f"grain_{fmt.name}_1080p", "H": H, "W": W, "frames_per_call": n, "groups": groups, "calls_per_group": 20, "input_sets": sets,
           "frame_bytes": nb, "apply_equals_torch": equal_apply, "stats_equal_torch": equal_stats, "stats_two_runs_same_bits": same}
    for name, key in (("apply", "apply"), ("stats", "stats"), ("frames_to_u8", "convert"), ("torch_apply", "apply_expr"), ("torch_stats", "stats_expr")):
        res[name + "_us_per_frame"] = 1e6 * med[key] / n
        res[name + "_us_per_frame_min_max"] = [1e6 * min(t[key]) / n, 1e6 * max(t[key]) / n]
    res.update(apply_over_frames_to_u8=med["apply"] / med["convert"], stats_over_frames_to_u8=med["stats"] / med["convert"],
               torch_over_apply=med["apply_expr"] / med["apply"], torch_over_stats=med["stats_expr"] / med["stats"],
               apply_bytes_per_s=2 * nb * n / med["apply"], stats_bytes_per_s=2 * nb * n / med["stats"])
    del clean, work, noisy, imgs
    torch.cuda.empty_cache()
    return res


# ---- the decoder loop and the closed loop --------------------------------------------------------------------------------------------
def bench_loop(anchors, steps, n_frames, repeats, dev):
    from bench_frames_out import headline_model
    pc, cube, pipe, bg = headline_model(anchors, steps, dev)
    fmt = FrameFormat("yuv420p")
    frames = [cube.get_dummy_frame(i) for i in range(8, 8 + n_frames)]
    p = G.GrainParams(source=fmt, **PARAMS)

    def run(grain):
        s = 0
        for f in fo.render_frames_u8(frames, pc, pipe, bg, fmt=fmt, to_host=True, grain=grain, first_frame=8):
            s += int(f[0])          # the frame is in host memory when it is handed out
        return s
    with torch.no_grad():
        for g in (None, p, None, p):
            run(g)
        torch.cuda.synchronize()
        rates = {"without": [], "with": []}
        for _ in range(repeats):          # alternated
            for name, g in (("without", None), ("with", p)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(g)
                torch.cuda.synchronize()
                rates[name].append(n_frames / (time.perf_counter() - t0))
        out = {"anchors": int(pc._anchor.shape[0]), "fit_steps": steps, "frames": n_frames, "repeats": repeats, "H": H, "W": W, "batch": 8}
        for name, r in rates.items():
            out[f"fps_{name}_grain"] = statistics.median(r)
            out[f"fps_{name}_grain_min_max"] = [min(r), max(r)]
        out["with_over_without"] = out["fps_with_grain"] / out["fps_without_grain"]
        # the closed loop: the clean clip's codes + known grain against the decoder's frames
        ids = list(range(8, 8 + min(n_frames, 16)))
        dec = torch.stack(list(fo.render_frames_u8([cube.get_dummy_frame(i) for i in ids], pc, pipe, bg, fmt=fmt, to_host=False)))
        src = G.apply_grain(fo.frames_to_u8([cube._image(i) for i in ids], fmt).contiguous(), H, W, fmt, p, frame_ids=ids)
        stats = G.grain_stats(src, dec, H, W, fmt)
        fitted = G.fit_grain(stats, seed=1, source=fmt)
        again = G.grain_stats(G.apply_grain(dec.clone(), H, W, fmt, fitted, frame_ids=ids), dec, H, W, fmt)
    sigma = lambda st: [[None if row[0] == 0 else max((row[2] - row[3] / 64.0) / (64.0 * row[0]), 0.0) ** 0.5 for row in plane]          # noqa: E731
                        for plane in st.cpu().tolist()]
    closed = {"frames": len(ids), "applied": {k: (list(map(list, v)) if k == "scale" else v) for k, v in PARAMS.items()},
              "fitted": fitted.summary(), "blocks_source_vs_decoded": G.blocks_used(stats), "blocks_per_bin_luma": [r[0] for r in stats[0].cpu().tolist()],
              "blocks_whole": [len(ids) * (H // 8) * (W // 8), len(ids) * (H // 16) * (W // 16), len(ids) * (H // 16) * (W // 16)],
              "flat_sigma_source_vs_decoded": sigma(stats), "flat_sigma_grained_vs_decoded": sigma(again),
              "blocks_grained_vs_decoded": G.blocks_used(again)}
    return out, closed


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=30)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--anchors", type=int, default=245_000)
    ap.add_argument("--fit-steps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_grain.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "bench_grain", "device": torch.cuda.get_device_name(dev), "kernel": []}
    with torch.no_grad():
        for depth in (8, 10):
            res["kernel"].append(bench_case(depth, 8, max(args.groups, 30), dev))
    if not args.no_loop:
        res["decoder_loop"], res["closed_loop"] = bench_loop(args.anchors, args.fit_steps, args.frames, args.repeats, dev)
    line = json.dumps(res)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
