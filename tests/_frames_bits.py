"""The bits of the frame kernels, pinned: SHA-256 digests of what ``frames_to_u8``, ``frames_from_u8``, ``plane_sse`` and
``picture_hash`` give on seeded inputs (tests/test_frames_bits_gpu.py compares them with tests/golden/frames_bits.json).

The tolerance tests of the frame stages allow half a code (output) or 2^-20 (input): a reordered multiply-add passes them.  A digest
does not.  The JSON is recorded with the library of the commit BEFORE a change of the kernels,

    GSVC_LIB_PATH=<that build's libgsvc_hip.so> python -m tests._frames_bits --record FILE --commit ID

and the test asserts that the library of the working tree reproduces every digest.

Inputs come from ``numpy.random.default_rng(seed)`` alone (its bit stream does not depend on the machine):
  * float images uniform in [-0.25, 1.25] with NaN, +-inf, 0, 1 and rounding ties planted (grey 0.5 is code 127.5 of 255 and 125.5 of
    16 + 219 Y; 0.25 / 0.75 tie at the deep full ranges);
  * code frames uniform over the whole word — deep codes above 2^d - 1 included, which the kernels do not mask.
Shapes: H in {2, 6} (six rows: a top-clamped, an interior and a bottom-clamped chroma row), W in {2, 20, 32, 36, 40} (2: edge; 20: deep
wide only; 32: wide everywhere, two 16-pixel lanes per row; 36: deep wide, 8-bit edge; 40: 8-bit 4:2:0 output wide, the other 8-bit
kernels edge), n in {1, 3}, one call of 17 frames (two launches), and one call on a buffer shifted by one sample (a wide-eligible W that
alignment alone sends to the edge path).  One digest covers the outputs of every matrix x range x rounding (or chroma mode) of a shape,
in the order of ``COMBOS``."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames_bits.json")
FORMATS = [("rgb24", 8)] + [(layout, depth) for layout in ("yuv444p", "yuv420p") for depth in (8, 10, 16)]
SHAPES = [(H, W, n) for H in (2, 6) for W in (2, 20, 32, 36, 40) for n in (1, 3)] + [(6, 32, 17)]
SHIFTED = (6, 32, 3)                       # the shape of the shifted-buffer call
COMBOS = [(m, r) for m in ("bt709", "bt601") for r in ("limited", "full")]
SPECIALS = [np.nan, np.inf, -np.inf, 0.0, 1.0, 0.5, 0.25, 0.75, 127.5 / 255.0, 0.5 / 255.0, 254.5 / 255.0, -0.0]


def _seed(H, W, n, salt):
    return ((salt * 100 + H) * 100 + W) * 100 + n


def images(H, W, n):
    """float32 [n, 3, H, W]."""
    rng = np.random.default_rng(_seed(H, W, n, 1))
    x = rng.uniform(-0.25, 1.25, (n, 3, H, W)).astype(np.float32)
    x[0, :, :2, :2] = 0.5                                        # one grey 2x2 block: luma and chroma ties
    flat = x.reshape(-1)
    flat[(5 + 7 * np.arange(len(SPECIALS))) % flat.size] = np.array(SPECIALS, np.float32)
    return x


def frame_samples(H, W, layout):
    return H * W * 3 // 2 if layout == "yuv420p" else 3 * H * W


def code_frames(H, W, n, layout, depth, salt=2):
    """uint8 [n, frame bytes]: every sample uniform over its whole 8- or 16-bit word."""
    rng = np.random.default_rng(_seed(H, W, n, salt) + depth)
    count = frame_samples(H, W, layout)
    if depth == 8:
        return rng.integers(0, 256, (n, count), dtype=np.uint8)
    return rng.integers(0, 65536, (n, count), dtype=np.uint16).astype("<u2").view(np.uint8).reshape(n, 2 * count)


def _digest(tensors):
    import torch
    flat = torch.cat([t.contiguous().reshape(-1).view(torch.uint8) for t in tensors])
    return hashlib.sha256(flat.cpu().numpy().tobytes()).hexdigest()


def _shifted(rows, shift):
    """The same rows in a buffer that starts ``shift`` bytes behind a 16-byte boundary."""
    import torch
    n, nb = rows.shape
    room = torch.zeros(n * nb + 16, dtype=torch.uint8, device=rows.device)
    view = room[shift:shift + n * nb].view(n, nb)
    view.copy_(rows)
    assert view.data_ptr() % 16 == shift
    return view


def out_digests(layout, depth):
    """{key: digest} of ``frames_to_u8`` for one layout and depth."""
    import torch

    from gsvc_amd import frames_out as fo
    got = {}
    for H, W, n, shift in [s + (0,) for s in SHAPES] + [SHIFTED + (2 if depth > 8 else 1,)]:
        dev = torch.from_numpy(images(H, W, n)).cuda()
        outs = []
        for matrix, rng in COMBOS:
            for rounding in ("trunc", "nearest"):
                fmt = fo.FrameFormat(layout, matrix, rng, rounding, depth)
                out = None
                if shift:
                    out = _shifted(torch.zeros((n, fo.frame_bytes(H, W, fmt)), dtype=torch.uint8, device="cuda"), shift)
                outs.append(fo.frames_to_u8(dev, fmt, out=out))
        got[f"out/{layout}/{depth}/{H}x{W}/n{n}" + ("/shifted" if shift else "")] = _digest(outs)
    return got


def in_digests(layout, depth):
    """{key: digest} of ``frames_from_u8`` for one layout and depth."""
    import torch

    from gsvc_amd import frames_in as fi
    from gsvc_amd.frames_out import FrameFormat
    got = {}
    for H, W, n, shift in [s + (0,) for s in SHAPES] + [SHIFTED + (2 if depth > 8 else 1,)]:
        dev = torch.from_numpy(code_frames(H, W, n, layout, depth)).cuda()
        if shift:
            dev = _shifted(dev, shift)
        outs = []
        for matrix, rng in COMBOS:
            for chroma in ("nearest", "bilinear"):
                outs.append(fi.frames_from_u8(dev, H, W, FrameFormat(layout, matrix, rng, depth=depth), chroma=chroma))
        got[f"in/{layout}/{depth}/{H}x{W}/n{n}" + ("/shifted" if shift else "")] = _digest(outs)
    return got


def sums_digests(layout, depth):
    """{key: digest} of ``plane_sse`` and ``picture_hash`` on 6 x 6 frames: planar layouts have their plane boundaries inside a 16-byte
    vector, rgb24 has 108 samples = two whole 48-sample units and a tail.  One frame (wide), three frames back to back (edge: the stride
    is no multiple of 16), three frames at a stride of a multiple of 16 (wide) and three frames shifted by one sample (edge)."""
    import torch

    from gsvc_amd import metrics
    from gsvc_amd.frames_out import FrameFormat
    H, W = 6, 6
    fmt = FrameFormat(layout, depth=depth)
    got = {}
    for n, how in ((1, "one"), (3, "tight"), (3, "padded"), (3, "shifted")):
        a = torch.from_numpy(code_frames(H, W, n, layout, depth, salt=3)).cuda()
        b = torch.from_numpy(code_frames(H, W, n, layout, depth, salt=4)).cuda()
        nb = a.shape[1]
        if how == "padded":
            stride = (nb + 15) // 16 * 16 + 16
            a, b = (torch.cat([t, t.new_zeros((n, stride - nb))], 1)[:, :nb] for t in (a, b))
            assert a.stride(0) % 16 == 0 and a.data_ptr() % 16 == 0
        elif how == "shifted":
            a, b = (_shifted(t, 2 if depth > 8 else 1) for t in (a, b))
        got[f"sse/{layout}/{depth}/{how}"] = _digest([metrics.plane_sse(a, b, H, W, fmt)])
        got[f"hash/{layout}/{depth}/{how}"] = _digest([metrics.picture_hash(a, H, W, fmt), metrics.picture_hash(b, H, W, fmt)])
    return got


def all_digests():
    got = {}
    for layout, depth in FORMATS:
        got.update(out_digests(layout, depth))
        got.update(in_digests(layout, depth))
        got.update(sums_digests(layout, depth))
    return got


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser(description="record the digests with the library GSVC_LIB_PATH names (the build before a change)")
    ap.add_argument("--record", required=True, metavar="FILE")
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    args = ap.parse_args()
    if not os.environ.get("GSVC_LIB_PATH"):
        raise SystemExit("--record takes the library of an earlier commit: set GSVC_LIB_PATH to its libgsvc_hip.so")
    with open(args.record, "w") as f:
        json.dump({"recorded_with": args.commit, "digests": all_digests()}, f, indent=0, sort_keys=True)
        f.write("\n")
