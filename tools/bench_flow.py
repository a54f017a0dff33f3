#!/usr/bin/env python3
"""What the optical-flow estimator costs (csrc/flow.hip: k_flow_blur, k_flow_warp, k_flow_solve) beside the same algorithm written as
tensor expressions, what its solver is bound by, and what the estimated flow does to a fit.  One process, one JSON line.

  estimate   per batch of n = 1, 4, 16 pairs of 1080 x 1920 lumas (the defaults of ``flow.FlowParams``): device-event time of groups of
             calls of ``flow.estimate_flow``, alternated in the same process with groups of ``torch_estimate`` below — the algorithm of
             include/gsvc_hip.h as tensor expressions (pad / slice / gather), kept in this tool, not in the package.  Per pair:
             ``kernel_ms_per_pair``, ``torch_expressions_ms_per_pair``, the ratio of the medians, ``faster_beyond_spread`` = the slowest
             kernel group is faster than the fastest tensor-expression group, ``max_difference`` in px between the two results, and the
             solver's share of the kernel path's device time (the library's per-kernel event timer, a run of its own).
  solver     one launch of k_flow_solve on the finest level, n = 16: 4 sweeps (what the estimate issues) and 1 sweep — the same tiles
             loaded and stored, a quarter of the arithmetic — with the launch's algorithmic bytes (five planes read over 64 x 64 staged
             cells per 56 x 56 owned ones, two written) and the bytes / s they give.  If one sweep costs what four do, the launch is
             bound by its traffic; if it costs a quarter, by its arithmetic.
  --rd       the effect on rate-distortion: ``tools/fit_synthetic.py`` at the README's 2 000-step setting, same seed, three ways —
             the synthetic video's analytic flow, ``--estimate-flow``, ``--optical-lambda 0`` — each in a process of its own: PSNR, bpp,
             and the estimated fields' mean endpoint error against the analytic ones.  The fits run with ``--payload-tol 1``: a
             measurement records the payload ratio, the tool's 2 % check on it is not what is measured here.
  --f32-error  no GPU: the float32 NumPy restatement against the float64 one on the GPU tests' cases (the figures of tests/_flow_ref.py).

    python tools/bench_flow.py [--groups 10] [--size 1080x1920] [--batches 1,4,16] [--rd] [--json profiles/flow.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gsvc_amd import _lib, flow  # noqa: E402

HBM_PEAK = 8.0e12          # bytes / s (MI355X)


# ---- the algorithm as tensor expressions ([n, h, w] float32 tensors) ---------------------------------------------------------------
def _pad(a, k):
    return F.pad(a.unsqueeze(1), (k, k, k, k), mode="replicate").squeeze(1)


def t_blur(a):
    h, w = a.shape[-2:]
    p = _pad(a, 2)[..., 2:w + 2]
    v = ((p[..., 0:h, :] + p[..., 4:h + 4, :]) + 4 * (p[..., 1:h + 1, :] + p[..., 3:h + 3, :]) + 6 * p[..., 2:h + 2, :]) * 0.0625
    p = _pad(v, 2)[..., 2:h + 2, :]
    return ((p[..., 0:w] + p[..., 4:w + 4]) + 4 * (p[..., 1:w + 1] + p[..., 3:w + 3]) + 6 * p[..., 2:w + 2]) * 0.0625


def t_pool(a):
    h, w = a.shape[-2] // 2 * 2, a.shape[-1] // 2 * 2
    a = a[..., :h, :w]
    return ((a[..., 0::2, 0::2] + a[..., 0::2, 1::2]) + (a[..., 1::2, 0::2] + a[..., 1::2, 1::2])) * 0.25


def t_bilinear(a, x, y):
    n, h, w = a.shape
    x, y = x.clamp(0, w - 1), y.clamp(0, h - 1)
    x0, y0 = x.floor().clamp(max=w - 2), y.floor().clamp(max=h - 2)
    fx, fy = x - x0, y - y0
    idx = (y0.long() * w + x0.long()).flatten(1)
    flat = a.flatten(1)
    a00, a01 = flat.gather(1, idx).view_as(x), flat.gather(1, idx + 1).view_as(x)
    a10, a11 = flat.gather(1, idx + w).view_as(x), flat.gather(1, idx + w + 1).view_as(x)
    top, bot = a00 + fx * (a01 - a00), a10 + fx * (a11 - a10)
    return top + fy * (bot - top)


def _grid(n, h, w, dev):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=dev), torch.arange(w, dtype=torch.float32, device=dev), indexing="ij")
    return xs.expand(n, h, w), ys.expand(n, h, w)


def t_upsample(c, h, w):
    xs, ys = _grid(c.shape[0], h, w, c.device)
    return 2 * t_bilinear(c, (xs + 0.5) * 0.5 - 0.5, (ys + 0.5) * 0.5 - 0.5)


def _gx(a):
    p = _pad(a, 1)
    return 0.5 * (p[..., 1:-1, 2:] - p[..., 1:-1, :-2])


def _gy(a):
    p = _pad(a, 1)
    return 0.5 * (p[..., 2:, 1:-1] - p[..., :-2, 1:-1])


def _mean4(a):
    p = _pad(a, 1)
    return 0.25 * ((p[..., 1:-1, :-2] + p[..., 1:-1, 2:]) + (p[..., :-2, 1:-1] + p[..., 2:, 1:-1]))


def torch_estimate(l0, l1, p=flow.FlowParams()):
    """[n, H, W] lumas -> [n, 2, H, W]."""
    P0, P1 = [t_blur(l0)], [t_blur(l1)]
    while min(P0[-1].shape[-2:]) // 2 >= p.min_side and len(P0) < p.max_levels:
        P0.append(t_blur(t_pool(P0[-1])))
        P1.append(t_blur(t_pool(P1[-1])))
    u = v = None
    for A, B in zip(reversed(P0), reversed(P1)):
        n, h, w = A.shape
        if u is None:
            u, v = torch.zeros_like(A), torch.zeros_like(A)
        else:
            u, v = t_upsample(u, h, w), t_upsample(v, h, w)
        xs, ys = _grid(n, h, w, A.device)
        Ax, Ay = _gx(A), _gy(A)
        for _ in range(p.warps):
            px, py = xs + u, ys + v
            Bw = t_bilinear(B, px, py)
            ox = torch.maximum(-px, px - (w - 1)).clamp(min=0)
            oy = torch.maximum(-py, py - (h - 1)).clamp(min=0)
            m = (1 - torch.maximum(ox, oy)).clamp(0, 1)
            Ix, Iy, It = m * (0.5 * (Ax + _gx(Bw))), m * (0.5 * (Ay + _gy(Bw))), m * (Bw - A)
            c = (It - Ix * u) - Iy * v
            den = 1 / ((p.alpha * p.alpha + Ix * Ix) + Iy * Iy)
            U, V = u, v
            for _ in range(p.iters):
                Ub, Vb = _mean4(U), _mean4(V)
                t = ((Ix * Ub + Iy * Vb) + c) * den
                U, V = Ub - Ix * t, Vb - Iy * t
            u = u + (U - u).clamp(-p.max_step, p.max_step)
            v = v + (V - v).clamp(-p.max_step, p.max_step)
    return torch.stack([u, v], 1)


# ---- measurements ------------------------------------------------------------------------------------------------------------------
def timed_group(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / calls          # seconds per call


def _lumas(n, H, W, dev):
    """n + 1 frames of a moving smooth texture in [0, 1]: pair k = frames k, k + 1, 2.3 px apart."""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
    g = torch.Generator().manual_seed(7)
    fx, fy = (torch.rand(2, 24, generator=g) * 0.5 - 0.25).tolist()
    ph = (torch.rand(24, generator=g) * 6.2832).tolist()
    frames = []
    for k in range(n + 1):
        t = sum(torch.sin(fx[j] * (xs - 2.0 * k) + fy[j] * (ys + 1.1 * k) + ph[j]) for j in range(24)) / 24
        frames.append(0.5 + 0.5 * t)
    return torch.stack(frames)


def bench_estimate(n, H, W, groups, dev):
    frames = _lumas(n, H, W, dev)
    a, b = frames[:-1].contiguous().unsqueeze(1), frames[1:].contiguous().unsqueeze(1)
    kernel = lambda: flow.estimate_flow(a, b)          # noqa: E731
    expr = lambda: torch_estimate(a[:, 0], b[:, 0])          # noqa: E731
    diff = float((kernel() - expr()).abs().max())
    _lib.profile_enable(True)
    kernel()
    prof = _lib.profile_collect()
    _lib.profile_enable(False)
    total = sum(ms for _, ms in prof.values())
    for _ in range(2):
        timed_group(kernel, 2)
        timed_group(expr, 1)
    tk, tt = [], []
    for _ in range(groups):          # alternated
        tk.append(timed_group(kernel, 2))
        tt.append(timed_group(expr, 1))
    k_med, t_med = statistics.median(tk), statistics.median(tt)
    return {"case": f"estimate_n{n}", "H": H, "W": W, "pairs_per_call": n, "groups": groups, "calls_per_group": [2, 1],
            "kernel_ms_per_pair": 1e3 * k_med / n, "kernel_ms_per_pair_min_max": [1e3 * min(tk) / n, 1e3 * max(tk) / n],
            "torch_expressions_ms_per_pair": 1e3 * t_med / n, "torch_expressions_ms_per_pair_min_max": [1e3 * min(tt) / n, 1e3 * max(tt) / n],
            "torch_over_kernel": t_med / k_med, "faster_beyond_spread": max(tk) < min(tt), "max_difference_px": diff,
            "kernel_launches_and_ms": {k: [c, ms] for k, (c, ms) in prof.items()}, "solver_share_of_kernel_time": prof["k_flow_solve"][1] / total}


def bench_solver(n, H, W, groups, dev):
    import ctypes as C
    L = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(3)
    U, V, c = (torch.randn((n, H, W), device=dev, generator=g) for _ in range(3))
    Ix, Iy = (0.1 * torch.randn((n, H, W), device=dev, generator=g) for _ in range(2))
    ou, ov = torch.empty_like(U), torch.empty_like(V)
    ws = torch.empty(int(L.gsvc_flow_solve_workspace_bytes(n, H, W)), dtype=torch.uint8, device=dev)
    st = _lib.current_stream(dev)

    def launch(sweeps):
        _lib.check(L.gsvc_flow_solve(U.data_ptr(), V.data_ptr(), Ix.data_ptr(), Iy.data_ptr(), c.data_ptr(), None, None, n, H, W, C.c_float(0.02), sweeps,
                                     C.c_float(1.0), ou.data_ptr(), ov.data_ptr(), ws.data_ptr(), st), "gsvc_flow_solve")
    out = {"case": "solver_launch", "H": H, "W": W, "pairs": n, "groups": groups, "launches_per_group": 20}
    tiles = -(-H // 56) * -(-W // 56)
    alg = n * (5 * tiles * 64 * 64 + 2 * H * W) * 4
    for sweeps in (4, 1):
        for _ in range(2):
            timed_group(lambda: launch(sweeps), 20)
        t = [timed_group(lambda: launch(sweeps), 20) for _ in range(groups)]
        out[f"us_{sweeps}_sweeps"] = 1e6 * statistics.median(t)
        out[f"us_{sweeps}_sweeps_min_max"] = [1e6 * min(t), 1e6 * max(t)]
    out["algorithmic_bytes"] = alg
    out["bytes_per_s_4_sweeps"] = alg / (out["us_4_sweeps"] * 1e-6)
    out["share_of_hbm_peak_8TBps_4_sweeps"] = out["bytes_per_s_4_sweeps"] / HBM_PEAK
    out["one_sweep_over_four_sweeps"] = out["us_1_sweeps"] / out["us_4_sweeps"]
    return out


def rd_effect(steps, timeout):
    """The three fits, one process each; stops at the first that fails."""
    tool = os.path.join(ROOT, "tools", "fit_synthetic.py")
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, extra in (("analytic_flow", []), ("estimated_flow", ["--estimate-flow"]), ("optical_lambda_0", ["--optical-lambda", "0"])):
            out = os.path.join(tmp, name + ".json")
            run = subprocess.run([sys.executable, tool, "--steps", str(steps), "--payload-tol", "1", "--json", out] + extra, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
            if run.returncode != 0:
                raise SystemExit(f"fit_synthetic.py {' '.join(extra)} failed ({run.returncode}):\n{run.stdout[-1500:]}\n{run.stderr[-2500:]}")
            log = json.load(open(out))
            ev = log["decoded_8bit_mlp"]
            rows[name] = {"psnr": ev["psnr"], "msssim": ev.get("msssim"), "bpp": log["bpp"], "total_bytes": log["total_bytes"], "anchors_coded": log["anchors_coded"],
                          "fit_seconds": log["fit_seconds"], "attribute_payload_vs_estimate": log["attribute_payload_vs_estimate"], "flow": log["flow"]}
            print(json.dumps({name: rows[name]}), flush=True)
    return {"tool": "tools/fit_synthetic.py", "steps": steps, "setting": "1080 x 1920, 64 frames, 100 000 anchors, lmbda 0.004, seed 0", "runs": rows}


def f32_error():
    import numpy as np

    from tests import _flow_ref as ref
    for case in ref.CASES:
        a, b = ref.case_inputs(case)
        e = np.abs(ref.estimate(a, b, np.float32).astype(np.float64) - ref.reference(case)).max()
        print(f"{case}: {e:.3e} (recorded {ref.F32_ERRORS[case]:.3e})")
    print(f"bound: 4 x {ref.F32_ERROR:.3e} = {ref.ESTIMATE_BOUND:.3e} px")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--rd", action="store_true")
    ap.add_argument("--rd-steps", type=int, default=2000)
    ap.add_argument("--rd-timeout", type=float, default=900.0, help="seconds per fit")
    ap.add_argument("--skip-timing", action="store_true", help="with --rd: the three fits only")
    ap.add_argument("--f32-error", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if args.f32_error:
        return f32_error()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flow.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    H, W = (int(v) for v in args.size.split("x"))
    res = {"tool": "bench_flow", "device": torch.cuda.get_device_name(dev), "params": vars(flow.FlowParams()).copy(), "rows": []}
    if not args.skip_timing:
        with torch.no_grad():
            for n in (int(v) for v in args.batches.split(",")):
                res["rows"].append(bench_estimate(n, H, W, args.groups, dev))
                torch.cuda.empty_cache()
            res["rows"].append(bench_solver(16, H, W, args.groups, dev))
        last = [r for r in res["rows"] if r["case"].startswith("estimate")][-1]
        res["largest_batch_faster_beyond_spread"] = last["faster_beyond_spread"]
        res["largest_batch_torch_over_kernel"] = last["torch_over_kernel"]
    if args.rd:
        torch.cuda.empty_cache()
        res["rd_effect"] = rd_effect(args.rd_steps, args.rd_timeout)
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
