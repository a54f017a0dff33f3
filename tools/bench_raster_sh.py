"""Cost of the rasterizer's optional sources at BASELINE.json configs[1] (1080p, 200 k Gaussians): forward and forward +
backward through GaussianRasterizer for colors_precomp + scale/rotation (the path GSVC takes), SH colours of degree 0, 1 and 3,
a precomputed 3-D covariance, and the depth / alpha maps (return_depth / return_alpha: aux_fwd, aux_fwd_bwd) next to their
emulation by a second render with colors_precomp = (z, 1, 0) on a black background (emulated_aux_fwd_bwd).  One process; hipEvents around each call after warm-ups; median of --repeats calls.
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

    # depth + alpha maps with the image (colors_precomp + scale/rotation, the image's rows above are colors_precomp_*)
    r = cases["colors_precomp"][0]
    r0 = make(0)                   # the emulation's second render: black background
    r.deferred = r0.deferred = True
    kw = dict(colors_precomp=d["colors"], scales=d["scales"], rotations=d["rotations"])
    gD, gA = torch.randn(1, H, W, device=dev), torch.randn(1, H, W, device=dev)
    M2 = torch.tensor(s["viewmatrix"], device=dev, dtype=torch.float32)[2]

    def aux_fwd():
        with torch.no_grad():
            r(means3D=d["means3D"], means2D=None, opacities=d["opacities"], return_depth=True, return_alpha=True, **kw)

    def aux_fwd_bwd():
        for t in d.values():
            t.grad = None
        m2 = torch.zeros_like(d["means3D"], requires_grad=True)
        image, _, _, depth, alpha = r(means3D=d["means3D"], means2D=m2, opacities=d["opacities"], return_depth=True,
                                      return_alpha=True, **kw)
        torch.autograd.backward([image, depth, alpha], [dL, gD, gA])

    def emulated_aux_fwd_bwd():
        for t in d.values():
            t.grad = None
        m2 = torch.zeros_like(d["means3D"], requires_grad=True)
        image, _, _ = r(means3D=d["means3D"], means2D=m2, opacities=d["opacities"], **kw)
        z = d["means3D"] @ M2[:3] + M2[3]
        maps, _, _ = r0(means3D=d["means3D"], means2D=m2, opacities=d["opacities"], scales=d["scales"], rotations=d["rotations"],
                        colors_precomp=torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], dim=1))
        torch.autograd.backward([image, maps[0], maps[1]], [dL, gD[0], gA[0]])
    with torch.no_grad():          # size the emulation's instance capacity too (same scene: same lists)
        r0.deferred = False
        r0(means3D=d["means3D"], means2D=None, opacities=d["opacities"], **kw)
        r0.deferred = True
    out["aux_fwd_us"] = round(timed(aux_fwd), 1)
    out["aux_fwd_bwd_us"] = round(timed(aux_fwd_bwd), 1)
    out["emulated_aux_fwd_bwd_us"] = round(timed(emulated_aux_fwd_bwd), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
