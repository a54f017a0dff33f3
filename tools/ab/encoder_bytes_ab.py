"""Does the encoder of one source tree write the bytes another tree's does?  Seven small encodes (``fit_setup.encode_gop`` with its option
groups, and tools/gsvc_encode.py --gop-frames), each in a process of its own under GSVC_DETERMINISTIC=1, with the SHA-256 of the file
and the log kept per tree; ``compare`` then puts several runs side by side.  Made for refactors of the encoder's host side: two trees
that share one built library (GSVC_LIB_PATH) must agree wherever one tree agrees with itself.

    python tools/ab/encoder_bytes_ab.py clips DIR                    the three test clips (noisy synthetic yuv420p: 8 and 16 frames of 64 x 48,
                                                                     8 frames of 96 x 64)
    python tools/ab/encoder_bytes_ab.py run TREE DIR OUT.json        every configuration with the gsvc_amd/ and tools/ of TREE, a child each
    python tools/ab/encoder_bytes_ab.py compare A.json B.json ...    a markdown table of the hashes; exit status 1 when a run whose
                                                                     neighbours agree with each other differs from them
"""
import hashlib
import json
import os
import subprocess
import sys

FIT = dict(steps=40, anchors=2000, slab_frames=8.0, densify_grad_threshold=2e-5)
CLIPS = {"a": (48, 64, 8), "long": (48, 64, 16), "wide": (64, 96, 8)}          # name: (H, W, frames)
CONFIGS = {1: ("a", {}),
           2: ("a", dict(init="detail")),
           3: ("a", dict(denoise="auto", film_grain=True, grain_seed=5, grain_max_residual=255, grain_flat_threshold=65535)),
           4: ("wide", dict(coded_size=(48, 32), denoise=2.0, frame_range=(0, 4))),
           5: ("a", dict(weighting="activity", weight_strength=0.75, roi=[(0, 0, 16, 16, 2.0)])),
           6: ("a", dict(loss_domain="yuv420")),
           7: ("long", ["--gop-frames", "8", "--denoise", "2.0"])}          # (a list: arguments of tools/gsvc_encode.py)
WALL_CLOCK = ("fit_seconds", "verify_decode_fps", "output")
CHILD_SECONDS = 240


def write_clips(folder):
    import numpy as np
    import torch

    from gsvc_amd.frame import SyntheticFrameCube
    from gsvc_amd.frames_out import FrameFormat, Y4MWriter, frames_to_u8
    fmt = FrameFormat("yuv420p")
    os.makedirs(folder, exist_ok=True)
    for name, (H, W, T) in CLIPS.items():
        cube = SyntheticFrameCube(H, W, T, seed=7, device="cuda")
        clean = frames_to_u8([cube._image(t) for t in range(T)], fmt).cpu().numpy().copy()
        noisy = np.clip(np.rint(clean + np.random.default_rng(3).normal(0.0, 2.0, clean.shape)), 0, 255).astype(np.uint8)
        with Y4MWriter(os.path.join(folder, name + ".y4m"), W, H, (25, 1), fmt) as sink:
            for fr in noisy:
                sink.write(torch.from_numpy(fr))


def encode_one(tree, folder, number):
    """Configuration ``number`` with the modules of ``tree`` -> {"sha256", "bytes", "log"} as one JSON line on stdout."""
    sys.path[:0] = [tree, os.path.join(tree, "tools")]
    import torch
    clip, what = CONFIGS[number]
    path = os.path.join(folder, clip + ".y4m")
    if isinstance(what, list):
        import gsvc_encode
        out = os.path.join(folder, f"out_{os.getpid()}.gsvs")
        log = gsvc_encode.main([path, "-o", out] + what + [x for k, v in FIT.items() for x in ("--" + k.replace("_", "-"), str(v))])
        with open(out, "rb") as f:
            blob = f.read()
        os.remove(out)
    else:
        from gsvc_amd.fit_setup import encode_gop
        blob, log = encode_gop(path, torch.device("cuda", 0), **what, **FIT)
    print("RESULT " + json.dumps({"sha256": hashlib.sha256(blob).hexdigest(), "bytes": len(blob), "log": log}))


def run_tree(tree, folder, out):
    """Every configuration in a child of its own; the first child that fails or runs out of time ends the run."""
    env = dict(os.environ, GSVC_DETERMINISTIC="1")
    results = {"tree": os.path.abspath(tree)}
    for number in CONFIGS:
        child = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "one", tree, folder, str(number)],
                               env=env, capture_output=True, text=True)
        lines = [ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")]
        if child.returncode != 0 or not lines:
            sys.stderr.write(child.stdout[-2000:] + child.stderr[-4000:])
            raise SystemExit(f"configuration {number} of {tree} ended with status {child.returncode}: nothing more is started")
        results[str(number)] = json.loads(lines[-1][len("RESULT "):])
        print(number, results[str(number)]["sha256"][:16], results[str(number)]["bytes"], flush=True)
        with open(out, "w") as f:
            json.dump(results, f, indent=1)


def without_wall_clock(log):
    if isinstance(log, dict):
        return {k: without_wall_clock(v) for k, v in log.items() if k not in WALL_CLOCK}
    return [without_wall_clock(v) for v in log] if isinstance(log, list) else log


def compare(paths):
    runs = [json.load(open(p)) for p in paths]
    print("| configuration | " + " | ".join(os.path.basename(p) for p in paths) + " | bytes | logs |\n|---|" + "---|" * (len(paths) + 2))
    bad = 0
    for number in CONFIGS:
        rows = [r[str(number)] for r in runs]
        same_bytes = len({r["sha256"] for r in rows}) == 1
        same_logs = all(without_wall_clock(r["log"]) == without_wall_clock(rows[0]["log"]) for r in rows)
        outer = rows[0]["sha256"] == rows[-1]["sha256"]          # the first and the last run are of one tree: does it agree with itself?
        bad += outer and not (same_bytes and same_logs)
        print(f"| {number} | " + " | ".join(r["sha256"][:16] for r in rows) + f" | {'equal' if same_bytes else 'DIFFERENT'}"
              f"{'' if outer else ' (first and last differ too)'} | {'equal' if same_logs else 'DIFFERENT'} |")
    return 1 if bad else 0


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "clips":
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
        write_clips(sys.argv[2])
    elif mode == "one":
        encode_one(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    elif mode == "run":
        run_tree(sys.argv[2], sys.argv[3], sys.argv[4])
    elif mode == "compare":
        sys.exit(compare(sys.argv[2:]))
    else:
        raise SystemExit(__doc__)
