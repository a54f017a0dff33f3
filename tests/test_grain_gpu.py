"""GPU tests of the film-grain kernels (csrc/grain.hip through gsvc_amd/grain.py): ``apply_grain`` and
``grain_stats`` against the numpy restatement of the docstring (tests/_grain_ref.py), bit for bit everywhere — sizes that are no
multiple of the 128 x 16 tile or of 4 samples, several tiles each way, row strides larger than a frame, batches over the 16-frame
launch, both layouts, depths 8 / 10 / 16, both ranges, the tap corners at the largest strength, codes at 0 and at the peak —, frame
indices that do not depend on the batch, the rejection thresholds of the statistics exactly at and one above, and the closed loop."""
import ctypes as C

import numpy as np
import pytest
import torch

from gsvc_amd import _lib
from gsvc_amd import grain as G
from gsvc_amd.frames_out import LAYOUTS, FrameFormat, frame_bytes
from tests import _grain_ref as ref

pytestmark = pytest.mark.gpu
# (H, W, bytes of padding behind every frame's row of the buffer)
SIZES = [(2, 2, 0), (38, 70, 0), (64, 96, 48), (64, 96, 6), (34, 260, 0)]


def _params(rng, fmt, strength=3000, kx=None, ky=None):
    scale = tuple(tuple(int(v) for v in rng.integers(0, strength + 1, 17)) for _ in range(3))
    return G.GrainParams(seed=int(rng.integers(0, 1 << 63)), scale=scale, kx=kx or tuple(int(v) for v in rng.integers(-32, 33, 3)),
                         ky=ky or tuple(int(v) for v in rng.integers(-32, 33, 3)), source=fmt)


def _buffer(rng, n, H, W, fmt, pad=0, kind="random"):
    """uint8 numpy [n, frame_bytes + pad]: codes over the whole 0 .. 2^depth - 1 (values outside the nominal range included)."""
    nb, peak = frame_bytes(H, W, fmt), (1 << fmt.depth) - 1
    samples = nb // (2 if fmt.depth > 8 else 1)
    codes = {"random": lambda: rng.integers(0, peak + 1, (n, samples)), "zero": lambda: np.zeros((n, samples), np.int64),
             "peak": lambda: np.full((n, samples), peak, np.int64)}[kind]()
    frames = codes.astype("<u2" if fmt.depth > 8 else np.uint8).view(np.uint8).reshape(n, nb)
    return np.concatenate([frames, rng.integers(0, 256, (n, pad), dtype=np.uint8)], axis=1) if pad else frames


def _apply(host, H, W, fmt, p, **kw):
    dev = torch.from_numpy(host.copy()).cuda()
    assert G.apply_grain(dev, H, W, fmt, p, **kw) is dev
    return dev.cpu().numpy()


def _ref(host, H, W, fmt, p, ids):
    return ref.apply_ref(host, H, W, fmt.layout, fmt.depth, fmt.range, p.seed, p.scale, p.kx, p.ky, ids)


# ---- apply_grain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("layout", ["yuv420p", "yuv444p"])
@pytest.mark.parametrize("H,W,pad", SIZES)
def test_apply_is_the_reference_bit_for_bit(H, W, pad, layout, depth):
    rng = np.random.default_rng(H * 1000 + W + depth + pad)
    fmt = FrameFormat(layout, range="limited" if (W // 2 + depth // 2 + (layout == "yuv444p")) % 2 else "full", depth=depth)
    p = _params(rng, fmt)
    host = _buffer(rng, 3, H, W, fmt, pad)
    got = _apply(host, H, W, fmt, p, first_frame=40)
    assert np.array_equal(got, _ref(host, H, W, fmt, p, [40, 41, 42]))
    nb = frame_bytes(H, W, fmt)
    assert np.array_equal(got[:, nb:], host[:, nb:])                          # the padding is untouched
    assert H * W < 100 or np.count_nonzero(got[:, :nb] != host[:, :nb]) > nb          # (and the frames are not)


@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("H,W,layout,depth,rng_name", [(38, 70, "yuv420p", 8, "limited"), (64, 96, "yuv444p", 10, "full")])
def test_apply_batches_cross_the_launch_of_16(n, H, W, layout, depth, rng_name):
    rng = np.random.default_rng(n + H)
    fmt = FrameFormat(layout, range=rng_name, depth=depth)
    p = _params(rng, fmt)
    host = _buffer(rng, n, H, W, fmt)
    got = _apply(host, H, W, fmt, p)
    assert np.array_equal(got, _ref(host, H, W, fmt, p, list(range(n))))
    if n == 1:                                            # one flat frame is a buffer of one
        flat = torch.from_numpy(host[0].copy()).cuda()
        G.apply_grain(flat, H, W, fmt, p)
        assert np.array_equal(flat.cpu().numpy(), got[0])


@pytest.mark.parametrize("kind", ["zero", "peak", "random"])
@pytest.mark.parametrize("depth,rng_name", [(8, "limited"), (8, "full"), (16, "limited"), (16, "full")])
def test_tap_corners_at_the_largest_strength_and_the_clamps(depth, rng_name, kind):
    rng = np.random.default_rng(depth)
    H, W = 34, 260
    for layout, kx, ky in (("yuv420p", (32, -32, 32), (32, 32, -32)), ("yuv444p", (-32, 32, -32), (-32, -32, 32))):
        fmt = FrameFormat(layout, range=rng_name, depth=depth)
        p = G.GrainParams(seed=77, scale=((65535,) * 17,) * 3, kx=kx, ky=ky, source=fmt)
        host = _buffer(rng, 2, H, W, fmt, kind=kind)
        got = _apply(host, H, W, fmt, p, first_frame=2 ** 32 - 2)
        assert np.array_equal(got, _ref(host, H, W, fmt, p, [2 ** 32 - 2, 2 ** 32 - 1]))
        planes = ref.plane_views(got[0], H, W, layout, depth)
        for k, plane in enumerate(planes):               # grain never leaves the nominal range, and never pulls a sample further out
            lo, hi = ref.nominal(k, depth, rng_name)
            code = {"zero": 0, "peak": (1 << depth) - 1}.get(kind)
            if code is not None:
                assert plane.min() >= min(lo, code) and plane.max() <= max(hi, code) and len(np.unique(plane)) > 1


def test_zero_strength_returns_the_input_bytes():
    rng = np.random.default_rng(1)
    for layout, depth in (("yuv420p", 8), ("yuv444p", 16)):
        fmt = FrameFormat(layout, depth=depth)
        host = _buffer(rng, 2, 38, 70, fmt)
        zero = G.GrainParams(seed=3, scale=((0,) * 17,) * 3, kx=(32, 32, 32), ky=(-32, 0, 5), source=fmt)
        assert np.array_equal(_apply(host, 38, 70, fmt, zero), host)
        # through the kernel too: only the luma plane has strength, the chroma planes come back as they went in
        luma_only = G.GrainParams(seed=3, scale=((900,) * 17, (0,) * 17, (0,) * 17), source=fmt)
        got = _apply(host, 38, 70, fmt, luma_only)
        nl = 38 * 70 * (2 if depth > 8 else 1)
        assert np.array_equal(got[:, nl:], host[:, nl:]) and not np.array_equal(got[:, :nl], host[:, :nl])
        assert np.array_equal(got, _ref(host, 38, 70, fmt, luma_only, [0, 1]))


def test_frame_indices_not_batches_decide_the_grain():
    rng = np.random.default_rng(5)
    H, W, fmt = 38, 70, FrameFormat("yuv420p")
    p = _params(rng, fmt)
    host = _buffer(rng, 9, H, W, fmt)
    whole = _apply(host, H, W, fmt, p)
    assert np.array_equal(_apply(host, H, W, fmt, p), whole)                                   # two runs: the same bytes
    split = np.concatenate([_apply(host[:5], H, W, fmt, p), _apply(host[5:], H, W, fmt, p, first_frame=5)])
    assert np.array_equal(split, whole)
    assert np.array_equal(_apply(host, H, W, fmt, p, frame_ids=list(range(9))), whole)
    ids = [8, 3, 3, 0, 7, 1, 2, 6, 5]
    picked = _apply(host[ids], H, W, fmt, p, frame_ids=ids)
    assert np.array_equal(picked, whole[ids])
    assert not np.array_equal(_apply(host, H, W, fmt, p, first_frame=1)[:-1], whole[:-1])
    with pytest.raises(ValueError):
        G.apply_grain(torch.from_numpy(host.copy()).cuda(), H, W, fmt, p, frame_ids=[0, 1])
    with pytest.raises(ValueError):
        G.apply_grain(torch.from_numpy(host.copy()).cuda(), H, W, fmt, p, first_frame=2 ** 32 - 3)


# ---- grain_stats -------------------------------------------------------------------------------------------------------------------
def _stats(src, dec, H, W, fmt, **kw):
    out = G.grain_stats(torch.from_numpy(src.copy()).cuda(), torch.from_numpy(dec.copy()).cuda(), H, W, fmt, **kw)
    assert out.dtype == torch.int64 and tuple(out.shape) == (3, 16, 6)
    return out.cpu().numpy()


def _noisy_pair(rng, n, H, W, fmt, pad=0):
    """dec: per sample a base code plus (0 .. 4) amp / 4, amp = 0, 2, 4, 5, 6, 4 for frame 0, 1, ..: the activity A of a block lies well
    below, around (amp 5: 112 x 1.9) and above the default threshold; src: dec plus -r .. r, r = 1, 5, 31, 33, 31, 5 (8-bit codes; times
    2^(depth - 8)): residuals below and, in frame 3, above the default bound."""
    up = 1 << (fmt.depth - 8)
    nb = frame_bytes(H, W, fmt)
    samples = nb // (2 if fmt.depth > 8 else 1)
    base = rng.integers(40, 200, (n, 1)) * up
    amp = np.array([0, 2, 4, 5, 6, 4])[np.arange(n) % 6][:, None]
    dec = base + rng.integers(0, 5, (n, samples)) * amp * up // 4
    res = np.array([1, 5, 31, 33, 31, 5])[np.arange(n) % 6][:, None] * up
    src = np.clip(dec + rng.integers(-1, 2, (n, samples)) * rng.integers(0, res + 1, (n, samples)), 0, (1 << fmt.depth) - 1)
    as_bytes = lambda a: a.astype("<u2" if fmt.depth > 8 else np.uint8).view(np.uint8).reshape(n, nb)          # noqa: E731
    tail = rng.integers(0, 256, (n, pad), dtype=np.uint8)
    return tuple(np.concatenate([as_bytes(a), tail], axis=1) if pad else as_bytes(a) for a in (src, dec))


@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("layout", ["yuv420p", "yuv444p"])
@pytest.mark.parametrize("H,W,pad", SIZES)
def test_stats_are_the_reference_bit_for_bit(H, W, pad, layout, depth):
    rng = np.random.default_rng(H + W + depth)
    fmt = FrameFormat(layout, depth=depth)
    src, dec = _noisy_pair(rng, 6, H, W, fmt, pad)
    got = _stats(src, dec, H, W, fmt)
    want = ref.stats_ref(src, dec, H, W, layout, depth, G.DEFAULT_FLAT_THRESHOLD, G.DEFAULT_MAX_RESIDUAL)
    assert np.array_equal(got, want)
    assert np.array_equal(_stats(src, dec, H, W, fmt), got)                                   # run to run
    # with nothing rejected every WHOLE block counts and no partial one
    everything = _stats(dec, dec, H, W, fmt, flat_threshold=65535, max_residual=0)
    ch, cw = (H // 2, W // 2) if layout == "yuv420p" else (H, W)
    assert everything[:, :, 0].sum(axis=1).tolist() == [6 * (H // 8) * (W // 8)] + [6 * (ch // 8) * (cw // 8)] * 2
    assert not everything[:, :, 1:].any()
    if (H, W) == (34, 260):
        assert want[:, :, 0].sum() > 0 and want[:, :, 0].sum() < everything[:, :, 0].sum()          # the case has blocks on both sides


@pytest.mark.parametrize("depth", [8, 10, 16])
def test_blocks_exactly_at_and_one_above_both_thresholds(depth):
    """yuv444p, 8 x 64: eight blocks per plane.  Block 0: A exactly at the threshold (a corner sample 112 up away: two differences);
    block 1: one above (an edge sample (224 up + 1) / 3 away: three differences); block 2: one residual exactly at the bound, block 3: one
    above it (negative); block 4: flat and equal.  Blocks 0, 2 and 4 count."""
    up, T, R = 1 << (depth - 8), G.DEFAULT_FLAT_THRESHOLD, G.DEFAULT_MAX_RESIDUAL
    H, W, fmt = 8, 64, FrameFormat("yuv444p", range="full", depth=depth)
    dec = np.full((3, H, W), 60 * up, np.int64)
    dec[:, 0, 0] += T * up // 2
    assert (T * up + 1) % 3 == 0
    dec[:, 0, 8 + 3] += (T * up + 1) // 3
    dec[:, :, 40:] += 3                                   # blocks 5 .. 7 differ from their left neighbour block, not inside
    src = dec.copy()
    src[:, 4, 16 + 5] += R * up
    src[:, 7, 24 + 7] -= R * up + 1
    as_bytes = lambda a: a.astype("<u2" if depth > 8 else np.uint8).view(np.uint8).reshape(1, -1)          # noqa: E731
    got = _stats(as_bytes(src), as_bytes(dec), H, W, fmt)
    assert np.array_equal(got, ref.stats_ref(as_bytes(src), as_bytes(dec), H, W, "yuv444p", depth, T, R))
    assert got[:, :, 0].sum(axis=1).tolist() == [6, 6, 6]                                      # 8 blocks less 1 and 3
    assert got[:, :, 2].sum(axis=1).tolist() == [(R * up) ** 2] * 3 and got[:, :, 1].sum(axis=1).tolist() == [R * up] * 3
    assert got[:, :, 3].sum(axis=1).tolist() == [(R * up) ** 2] * 3 and not got[:, :, 4:].any()
    one_less = _stats(as_bytes(src), as_bytes(dec), H, W, fmt, flat_threshold=T - 1, max_residual=R - 1)
    assert one_less[:, :, 0].sum(axis=1).tolist() == [4, 4, 4]


def test_chroma_bins_come_from_the_16x16_luma_region():
    """yuv420p 32 x 32: four chroma blocks per plane.  The luma region under chroma block (0, 0) holds the 8 x 8 values 16, 16, 16, 208: its
    mean 64 is bin 4, a bin none of its luma blocks is in; the others are flat at 40 (bin 2), 250 (bin 15) and 0 (bin 0)."""
    H = W = 32
    fmt = FrameFormat("yuv420p", range="full")
    luma = np.zeros((H, W), np.int64)
    luma[:16, :16] = 16
    luma[8:16, 8:16] = 208
    luma[:16, 16:] = 40
    luma[16:, :16] = 250
    dec = np.concatenate([luma.reshape(-1), np.full(2 * 16 * 16, 100)]).astype(np.uint8)[None]
    src = dec.copy()
    src[0, H * W:] += 1
    got = _stats(src, dec, H, W, fmt, flat_threshold=0)
    assert np.array_equal(got, ref.stats_ref(src, dec, H, W, "yuv420p", 8, 0, 32))
    for p in (1, 2):
        assert np.nonzero(got[p, :, 0])[0].tolist() == [0, 2, 4, 15] and got[p, 4].tolist() == [1, 64, 64, 4096, 56, 56]
    assert np.nonzero(got[0, :, 0])[0].tolist() == [0, 1, 2, 13, 15] and got[0, :, 0].sum() == 16 and not got[0, :, 1:].any()


def test_closed_loop_on_the_device_returns_the_parameters():
    c = ref.closed_loop_case()
    fmt = FrameFormat(c["layout"], range=c["range"], depth=c["depth"])
    p = G.GrainParams(seed=c["seed"], scale=c["scale"], kx=c["kx"], ky=c["ky"], source=fmt)
    dec = torch.from_numpy(c["dec"].copy()).cuda()
    src = G.apply_grain(dec.clone(), c["H"], c["W"], fmt, p, frame_ids=c["frame_ids"])
    stats = G.grain_stats(src, dec, c["H"], c["W"], fmt, flat_threshold=0)
    got = G.fit_grain(stats, seed=1, source=fmt)
    rel, tap = ref.recovery_error(c, got.scale, got.kx, got.ky)
    print(f"closed loop on the device: strengths within {rel:.5f}, taps within {tap}")
    assert rel <= ref.CLOSED_LOOP_BOUND[0] and tap <= ref.CLOSED_LOOP_BOUND[1]
    assert G.blocks_used(stats) == [4096, 1024, 1024]


# ---- the C-ABI's refusals ------------------------------------------------------------------------------------------------------------
def test_abi_error_returns():
    L = _lib.lib()
    H, W = 16, 32
    buf = torch.zeros((17, 2 * frame_bytes(H, W, FrameFormat("yuv444p")) + 8), dtype=torch.uint8, device="cuda")
    out = torch.zeros((3, 16, 6), dtype=torch.int64, device="cuda")
    before = buf.clone()
    c = G.GrainParams(seed=1, scale=((500,) * 17,) * 3).as_c()
    ids = (C.c_int64 * 17)(*range(17))
    Y420, Y444, RGB = LAYOUTS["yuv420p"], LAYOUTS["yuv444p"], LAYOUTS["rgb24"]
    stride = int(buf.stride(0))

    def apply(n=1, H=H, W=W, layout=Y420, depth=8, rng=0, stride=stride, params=c, ids=ids, ptr=buf.data_ptr()):
        rc = L.gsvc_grain_apply(ptr, stride, n, H, W, layout, depth, rng, C.byref(params) if params is not None else None, ids, None)
        return rc, L.gsvc_last_error().decode()

    def stats(n=1, H=H, W=W, layout=Y420, depth=8, flat=224, res=32, sa=stride, sb=stride, a=buf.data_ptr(), b=buf.data_ptr(), o=out.data_ptr()):
        rc = L.gsvc_grain_stats(a, sa, b, sb, n, H, W, layout, depth, flat, res, o, None)
        return rc, L.gsvc_last_error().decode()

    bad_tap = G.GrainParams(seed=1, scale=((500,) * 17,) * 3).as_c()
    bad_tap.kx[1] = 33
    bad_id = (C.c_int64 * 17)(*([0] * 16 + [0]))
    bad_id[0] = 1 << 32
    for call, text in ((apply(H=15), "even"), (apply(W=31), "even"), (apply(n=17), "n must be"), (apply(n=0), "n must be"),
                       (apply(stride=frame_bytes(H, W, FrameFormat("yuv420p")) - 1), "shorter than a frame"),
                       (apply(depth=10, stride=stride - 1, n=2), "multiple of 2"), (apply(depth=10, ptr=buf.data_ptr() + 1), "2-byte aligned"),
                       (apply(layout=RGB), "rgb24"), (apply(layout=7), "layout"), (apply(depth=9), "depth"), (apply(rng=2), "range"),
                       (apply(params=bad_tap), "taps"), (apply(ids=bad_id), "frame index"), (apply(params=None), "NULL"), (apply(ptr=None), "NULL"),
                       (stats(H=15), "even"), (stats(layout=RGB), "rgb24"), (stats(depth=11), "depth"), (stats(flat=-1), "flat_threshold"),
                       (stats(flat=65536), "flat_threshold"), (stats(res=256), "max_residual"), (stats(n=0), "n must be"),
                       (stats(sb=10), "shorter than a frame"), (stats(depth=16, sa=stride - 1, n=2), "multiple of 2"),
                       (stats(o=out.data_ptr() + 4), "8-byte aligned"), (stats(b=None), "NULL")):
        assert call[0] == -1 and text in call[1], (call, text)
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and not out.any()                      # nothing was launched
    assert apply(n=16, layout=Y444)[0] == 0 and stats(n=17, layout=Y444, depth=16)[0] == 0
    torch.cuda.synchronize()
