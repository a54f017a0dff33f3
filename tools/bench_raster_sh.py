"""Cost of the rasterizer's optional sources at BASELINE.json configs[1] (1080p, 200 k Gaussians): forward and forward +
backward through GaussianRasterizer for colors_precomp + scale/rotation (the path GSVC takes), SH colours of degree 0, 1 and 3,
and a precomputed 3-D covariance.  One process; hipEvents around each call after warm-ups; median of --repeats calls.
Prints one JSON line (microseconds)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsvc_amd import rasterizer, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--gaussians", type=int, default=200_000)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    assert args.repeats >= 20, "the median of at least 20 calls"
    dev = torch.device("cuda:0")
    H, W, P, T = args.height, args.width, args.gaussians, 600
    sc = synthetic.raster_scene(P, H=H, W=W, T=T, seed=2026, window_frames=16, frame_id=T // 2, sigma_px=(0.5, 4.0))
    s = sc["settings"]
    campos = (0.0, 0.0, float(s["z_cam"]) - 3.0 * float(s["threshold"]))

    def make(sh_degree):
        rs = rasterizer.GaussianRasterizationSettings(
            image_height=H, image_width=W, x_min=s["x_min"], y_min=s["y_min"], scale=s["scale"], threshold=s["threshold"],
            bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=torch.tensor(s["viewmatrix"]), sh_degree=sh_degree,
            campos=torch.tensor(campos), prefiltered=False, debug=False)
        return rasterizer.GaussianRasterizer(raster_settings=rs)

    d = {k: torch.tensor(sc[k], device=dev).requires_grad_(True) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
    rng = np.random.default_rng(1)
    shs = torch.tensor((rng.standard_normal((P, 16, 3)) * 0.3).astype(np.float32), device=dev, requires_grad=True)
    with torch.no_grad():
        q = d["rotations"] / d["rotations"].norm(dim=1, keepdim=True)
        r, x, y, z = q.unbind(1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)
        L = R * d["scales"][:, None, :]
        S = L @ L.transpose(1, 2)
        cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1).contiguous()
    cov.requires_grad_(True)
    dL = torch.randn(3, H, W, device=dev)

    cases = {
        "colors_precomp": (make(0), dict(colors_precomp=d["colors"], scales=d["scales"], rotations=d["rotations"])),
        "sh_deg0": (make(0), dict(shs=shs, scales=d["scales"], rotations=d["rotations"])),
        "sh_deg1": (make(1), dict(shs=shs, scales=d["scales"], rotations=d["rotations"])),
        "sh_deg3": (make(3), dict(shs=shs, scales=d["scales"], rotations=d["rotations"])),
        "cov3D_precomp": (make(0), dict(colors_precomp=d["colors"], cov3D_precomp=cov)),
    }

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(ts))

    out = {"H": H, "W": W, "P": P, "repeats": args.repeats}
    for name, (r, kw) in cases.items():
        with torch.no_grad():      # one synchronised call first: it sizes the instance capacity for this render
            r(means3D=d["means3D"], means2D=None, opacities=d["opacities"], **kw)
        r.deferred = True          # the counters stay on the device: no host sync inside the timed call

        def fwd():
            with torch.no_grad():
                r(means3D=d["means3D"], means2D=None, opacities=d["opacities"], **kw)

        def fwd_bwd():
            for t in list(d.values()) + [shs, cov]:
                t.grad = None
            m2 = torch.zeros_like(d["means3D"], requires_grad=True)
            image, _, _ = r(means3D=d["means3D"], means2D=m2, opacities=d["opacities"], **kw)
            image.backward(dL)
        out[f"{name}_fwd_us"] = round(timed(fwd), 1)
        out[f"{name}_fwd_bwd_us"] = round(timed(fwd_bwd), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
