"""GPU tests of the temporal prefilter's kernels (csrc/tfilter.hip through gsvc_amd/tfilter.py): ``temporal_filter``
and ``noise_sums`` against the numpy restatement of the docstring (tests/_tfilter_ref.py), bit for bit — sizes with partial 8 x 8 blocks
on both edges, padded frame strides whose guard bytes stay untouched, both layouts, depths 8 / 10 / 16, every frame of a short clip as
the target so that neighbours are missing on both sides, flows with exact rounding ties, huge finite values and vectors that leave the
picture over every edge —, the arithmetic's extremes, batches over the 16-frame launch, ``denoise_frames`` end to end, and the C-ABI's
refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from gsvc_amd import _lib
from gsvc_amd import tfilter as TF
from gsvc_amd.frames_out import LAYOUTS, FrameFormat, frame_bytes
from tests import _tfilter_ref as ref

pytestmark = pytest.mark.gpu
SIZES = [(16, 24), (38, 70), (64, 96)]          # (38, 70): partial blocks at the right and at the bottom
LUT_B, LUT_P = TF.default_luts()
PAD = 48                                        # guard bytes behind every frame of a buffer


def _clip(rng, T, H, W, fmt, pad=PAD):
    """uint8 numpy [T, frame_bytes + pad]: a smooth picture per plane that drifts from frame to frame, plus noise whose strength rises
    from left to right (blocks of every weight), plus a band of codes over the whole range; the guard bytes are random."""
    nb, peak, up = frame_bytes(H, W, fmt), (1 << fmt.depth) - 1, 1 << (fmt.depth - 8)
    ch, cw = (H // 2, W // 2) if fmt.layout == "yuv420p" else (H, W)
    frames = []
    for t in range(T):
        planes = []
        for h, w in ((H, W), (ch, cw), (ch, cw)):
            y, x = np.mgrid[0:h, 0:w].astype(np.float64)
            s = W / w
            base = 120.0 + 60.0 * np.sin((x * s + 0.3 * t) / 7.0) * np.cos(y * s / 5.0) + 0.4 * x * s
            noise = rng.normal(0.0, 1.0, (h, w)) * (0.2 + 6.0 * x / w)
            p = np.clip(np.rint((base + noise) * up), 0, peak).astype(np.int64)
            p[h // 2:h // 2 + 3] = rng.integers(0, peak + 1, (3, w))
            planes.append(p.reshape(-1))
        frames.append(np.concatenate(planes))
    codes = ref.as_bytes(np.stack(frames), fmt.depth)
    assert codes.shape == (T, nb)
    return np.concatenate([codes, rng.integers(0, 256, (T, pad), dtype=np.uint8)], axis=1) if pad else codes


def _flows(rng, n, H, W):
    """float32 [n, 4, 2, H, W]: multiples of 1 / 8 (every rounding tie of 4 f among them), most within +-1 px and a quarter up to +-6 px, a band along every edge that
    points out of the picture, and a sprinkling of +-1e9."""
    f = (rng.integers(-8, 9, (n, 4, 2, H, W)) / 8.0).astype(np.float32)
    far = rng.random((n, 4, 1, H, W)) < 0.25
    f = np.where(far, (rng.integers(-48, 49, f.shape) / 8.0).astype(np.float32), f)
    f[:, :, 0, :, :3] -= 9.0
    f[:, :, 0, :, -3:] += 9.0
    f[:, :, 1, :3, :] -= 9.0
    f[:, :, 1, -3:, :] += 9.0
    huge = rng.random(f.shape) < 0.01
    f[huge] = np.where(rng.random(int(huge.sum())) < 0.5, np.float32(1e9), np.float32(-1e9))
    return f


def _run(host, H, W, fmt, flows, q, params=None, first=0, pad=PAD):
    """temporal_filter into a padded output buffer -> (uint8 numpy [n, frame_bytes], the guard bytes were left alone)."""
    nb = frame_bytes(H, W, fmt)
    dev = torch.from_numpy(host.copy()).cuda()
    out = torch.full((flows.shape[0], nb + pad), 0xA5, dtype=torch.uint8, device="cuda")
    got = TF.temporal_filter(dev, H, W, fmt, torch.from_numpy(flows).cuda(), q, params, out=out, first=first)
    assert got is out
    got = out.cpu().numpy()
    assert np.array_equal(dev.cpu().numpy(), host)                                     # the clip is only read
    return got[:, :nb], bool((got[:, nb:] == 0xA5).all())


@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("layout", ["yuv420p", "yuv444p"])
@pytest.mark.parametrize("H,W", SIZES)
def test_filter_is_the_reference_bit_for_bit(H, W, layout, depth):
    rng = np.random.default_rng(H * 1000 + W + depth)
    fmt, T, up = FrameFormat(layout, depth=depth), 5, 1 << (depth - 8)
    host = _clip(rng, T, H, W, fmt)
    flows = _flows(rng, T, H, W)
    q, wide = (40 * up, 24 * up + 1, 56 * up + 3), tuple(min(v, TF.Q_MAX) for v in (400 * up + 7, 240 * up + 1, 560 * up + 3))
    got, guard = _run(host, H, W, fmt, flows, wide)          # (random vectors predict badly: a wide q keeps the weights off zero)
    want = ref.filter_frames(host, H, W, layout, depth, flows, wide, TF.DEFAULT_WT, LUT_B, LUT_P)
    assert np.array_equal(got, want)
    assert guard
    nb = frame_bytes(H, W, fmt)
    # a zero flow as well: the static case, where most neighbours are accepted
    still = np.zeros_like(flows)
    got0, _ = _run(host, H, W, fmt, still, q)
    assert np.array_equal(got0, ref.filter_frames(host, H, W, layout, depth, still, q, TF.DEFAULT_WT, LUT_B, LUT_P))
    samples = nb // (2 if depth > 8 else 1)
    changed = lambda a: np.count_nonzero(ref.as_codes(a, depth) != ref.as_codes(host[:, :nb], depth))          # noqa: E731
    assert changed(got0) > T * samples // 10 and changed(got) > T * samples // 2           # (both runs did filter)


def test_missing_neighbour_slots_are_never_read():
    """The slots of neighbours outside the clip hold NaN: were one read, the result would change."""
    rng = np.random.default_rng(4)
    H, W, fmt = 38, 70, FrameFormat("yuv420p")
    host = _clip(rng, 3, H, W, fmt)
    flows = _flows(rng, 3, H, W)
    want, _ = _run(host, H, W, fmt, flows, 48)
    poisoned = flows.copy()
    for k in range(3):
        for j, d in enumerate(TF.OFFSETS):
            if not 0 <= k + d < 3:
                poisoned[k, j] = np.nan
    got, _ = _run(host, H, W, fmt, poisoned, 48)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("q", [1, 65535])
@pytest.mark.parametrize("layout", ["yuv420p", "yuv444p"])
def test_largest_sse_and_saturated_indices(layout, q):
    """Depth 16, every plane a 0 / 65535 checkerboard whose phase alternates from frame to frame, zero flow: every prediction is the
    opposite code, the block SSE is 64 x 65535^2 and both indices saturate at 63 for q = 1 and for q = 65535."""
    H, W, T, fmt = 24, 40, 4, FrameFormat(layout, depth=16)
    ch, cw = (H // 2, W // 2) if layout == "yuv420p" else (H, W)
    frames = []
    for t in range(T):
        planes = [(((np.add.outer(np.arange(h), np.arange(w)) + t) % 2) * 65535).reshape(-1) for h, w in ((H, W), (ch, cw), (ch, cw))]
        frames.append(np.concatenate(planes))
    host = ref.as_bytes(np.stack(frames), 16)
    flows = np.zeros((T, 4, 2, H, W), np.float32)
    clip = [tuple(p.astype(np.int64) for p in ref.plane_views(f, H, W, layout, 16)) for f in host]
    odd = ref.predict(clip[1][0], 0, 0, 4)
    assert ref.block_index(clip[0][0], odd, q).min() == 63 and int(((clip[0][0] - odd) ** 2)[:8, :8].sum()) == 64 * 65535 ** 2
    got, _ = _run(host, H, W, fmt, flows, q, pad=0)
    assert np.array_equal(got, ref.filter_frames(host, H, W, layout, 16, flows, (q,) * 3, TF.DEFAULT_WT, LUT_B, LUT_P))
    # tables that do not fall: the neighbours at distance 2 are in phase, those at distance 1 are not, all at their full weight
    flat = TF.TemporalFilterParams(wt=(256, 256), lut_b=(256,) * 64, lut_p=(256,) * 64)
    got, _ = _run(host, H, W, fmt, flows, q, flat, pad=0)
    assert np.array_equal(got, ref.filter_frames(host, H, W, layout, 16, flows, (q,) * 3, flat.wt, flat.lut_b, flat.lut_p))
    assert not np.array_equal(got, host)


def test_block_index_exactly_at_and_one_below_a_step():
    """yuv444p 8 x 16, two blocks, q = 32: n_B q^2 = 2^16, so i_b = SSE // 32.  Block 0 differs from its prediction by 23, 3, 2, 1, 1
    (SSE 544 = 17 x 32: the first index at which LUT_B has fallen), block 1 by 23, 3, 2, 1 (SSE 543: index 16, full weight)."""
    H, W, fmt = 8, 16, FrameFormat("yuv444p", range="full")
    cur = np.full((3, H, W), 100, np.int64)
    nxt = cur.copy()
    for k, dv in enumerate((23, 3, 2, 1, 1)):
        nxt[0, 1 + k, 2] += dv
    for k, dv in enumerate((23, 3, 2, 1)):
        nxt[0, 1 + k, 8 + 3] -= dv
    host = ref.as_bytes(np.stack([cur.reshape(-1), nxt.reshape(-1)]), 8)
    flows = np.zeros((2, 4, 2, H, W), np.float32)
    ib = ref.block_index(cur[0], nxt[0], 32)
    assert ib[0, 0] == 17 and ib[0, 8] == 16 and LUT_B[17] < LUT_B[16]
    got, _ = _run(host, H, W, fmt, flows, (32, 32, 32), pad=0)
    want = ref.filter_frames(host, H, W, "yuv444p", 8, flows, (32, 32, 32), TF.DEFAULT_WT, LUT_B, LUT_P)
    assert np.array_equal(got, want)
    # the same at depth 10 with q = 128 and differences four times as large: the same indices
    host10 = ref.as_bytes(4 * np.stack([cur.reshape(-1), nxt.reshape(-1)]), 10)
    fmt10 = FrameFormat("yuv444p", range="full", depth=10)
    assert ref.block_index(4 * cur[0], 4 * nxt[0], 128)[0, ::8].tolist() == [17, 16]
    got10, _ = _run(host10, H, W, fmt10, flows, 128, pad=0)
    assert np.array_equal(got10, ref.filter_frames(host10, H, W, "yuv444p", 10, flows, (128,) * 3, TF.DEFAULT_WT, LUT_B, LUT_P))


@pytest.mark.parametrize("n", [1, 3, 17])
def test_batches_cross_the_launch_of_16(n):
    rng = np.random.default_rng(n)
    H, W, fmt = 38, 70, FrameFormat("yuv420p")
    host = _clip(rng, n, H, W, fmt)
    flows = _flows(rng, n, H, W)
    q = (40, 30, 50)
    whole, guard = _run(host, H, W, fmt, flows, q)
    assert guard and np.array_equal(whole, ref.filter_frames(host, H, W, "yuv420p", 8, flows, q, TF.DEFAULT_WT, LUT_B, LUT_P))
    assert np.array_equal(_run(host, H, W, fmt, flows, q)[0], whole)                               # two runs: the same bytes
    singles = np.concatenate([_run(host, H, W, fmt, flows[k:k + 1], q, first=k)[0] for k in range(n)])
    assert np.array_equal(singles, whole)
    chunks = np.concatenate([_run(host, H, W, fmt, flows[k:k + 5], q, first=k)[0] for k in range(0, n, 5)])
    assert np.array_equal(chunks, whole)                                                           # the caller's chunking does not matter
    if n == 1:
        assert np.array_equal(whole, host[:, :frame_bytes(H, W, fmt)])                             # one frame: no neighbour
    with pytest.raises(ValueError):
        TF.temporal_filter(torch.from_numpy(host.copy()).cuda(), H, W, fmt, torch.from_numpy(flows).cuda(), q, first=1)


# ---- noise_sums ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("layout", ["yuv420p", "yuv444p"])
@pytest.mark.parametrize("H,W", SIZES + [(10, 520)])
def test_noise_sums_are_the_reference_bit_for_bit(H, W, layout, depth):
    rng = np.random.default_rng(H + W + depth)
    fmt, n = FrameFormat(layout, depth=depth), 18
    nb, peak = frame_bytes(H, W, fmt), (1 << depth) - 1
    codes = rng.integers(0, peak + 1, (n, nb // (2 if depth > 8 else 1)))
    host = np.concatenate([ref.as_bytes(codes, depth), rng.integers(0, 256, (n, PAD), dtype=np.uint8)], axis=1)
    dev = torch.from_numpy(host.copy()).cuda()
    got = TF.noise_sums(dev, H, W, fmt)
    assert got.dtype == torch.int64 and tuple(got.shape) == (n, 3)
    assert np.array_equal(got.cpu().numpy(), ref.noise_sums_ref(host, H, W, layout, depth))
    assert torch.equal(TF.noise_sums(dev, H, W, fmt), got)                                         # run to run
    assert torch.equal(TF.noise_sums(dev[3], H, W, fmt)[0], got[3])                                # one flat frame


def test_noise_sums_of_a_constant_plane_and_of_the_checkerboard():
    H, W = 38, 70
    for layout in ("yuv420p", "yuv444p"):
        fmt = FrameFormat(layout, depth=16)
        ch, cw = (H // 2, W // 2) if layout == "yuv420p" else (H, W)
        samples = H * W + 2 * ch * cw
        flat = torch.from_numpy(ref.as_bytes(np.full((2, samples), 65535), 16)).cuda()
        assert not TF.noise_sums(flat, H, W, fmt).any()
        board = np.concatenate([((np.add.outer(np.arange(h), np.arange(w)) % 2) * 65535).reshape(-1) for h, w in ((H, W), (ch, cw), (ch, cw))])
        got = TF.noise_sums(torch.from_numpy(ref.as_bytes(board[None], 16)).cuda(), H, W, fmt)
        inner = TF.interior_samples(H, W, fmt)
        assert got.cpu().tolist() == [[8 * 65535 * v for v in inner]]                              # the largest sum there is


# ---- denoise_frames -----------------------------------------------------------------------------------------------------------------
def test_denoise_frames_is_the_reference_fed_the_same_flows():
    H, W, T, fmt = 64, 96, 6, FrameFormat("yuv420p")
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)

    def picture(t, h, w, s):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64) * s
        xx = xx - 1.5 * t
        return 120.0 + 50.0 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + 25.0 * np.sin((xx + yy) / 13.0)

    clean = np.stack([np.concatenate([np.rint(picture(t, H, W, 1)).reshape(-1), np.rint(picture(t, H // 2, W // 2, 2)).reshape(-1),
                                      np.rint(picture(t, H // 2, W // 2, 2)).reshape(-1)]) for t in range(T)]).astype(np.int64)
    noisy = np.clip(np.rint(clean + rng.normal(0.0, 3.0, clean.shape)), 0, 255).astype(np.int64)
    host = ref.as_bytes(noisy, 8)
    dev = torch.from_numpy(host.copy()).cuda()
    out, log = TF.denoise_frames(dev, H, W, fmt, chunk=4)
    assert log["source"] == "auto" and len(log["sigma"]) == 3 and all(1 <= v <= 65535 for v in log["q"]) and np.isfinite(log["psnr_y"])
    lumas = TF.code_lumas(dev, H, W, fmt)
    assert lumas.dtype == torch.float32 and tuple(lumas.shape) == (T, H, W)
    # (the device may multiply by the rounded reciprocal: two roundings of 2^-24 each on values of at most 1)
    assert np.abs(lumas.cpu().numpy().astype(np.float64) - noisy[:, :H * W].reshape(T, H, W) / 255.0).max() <= 2.0 ** -23
    flows = TF.neighbour_flows(lumas, 0, T)
    assert torch.equal(torch.cat([TF.neighbour_flows(lumas, 0, 4), TF.neighbour_flows(lumas, 4, 2)]), flows)          # chunks: the same flows
    want = ref.filter_frames(host, H, W, "yuv420p", 8, flows.cpu().numpy(), log["q"], TF.DEFAULT_WT, LUT_B, LUT_P)
    got = out.cpu().numpy()
    assert np.array_equal(got, want)
    assert log["q"] == list(TF.noise_strength(ref.noise_sums_ref(host, H, W, "yuv420p", 8), H, W, fmt)[1])
    mse_in = float(((noisy - clean)[:, :H * W].astype(np.float64) ** 2).mean())
    mse_out = float(((got.astype(np.int64) - clean)[:, :H * W].astype(np.float64) ** 2).mean())
    print(f"denoise_frames 64 x 96, sigma 3: estimated sigma {log['sigma'][0]:.2f}, q {log['q']}, output MSE / input MSE = {mse_out / mse_in:.3f}, "
          f"PSNR-Y out vs in {log['psnr_y']:.2f} dB")
    assert mse_out < mse_in
    # a given sigma, and a gain
    _, given = TF.denoise_frames(dev, H, W, fmt, sigma=2.0, gain=1.5)
    assert given["source"] == "given" and given["q"] == [48, 48, 48]
    # a GOP of one frame returns its input
    one, log1 = TF.denoise_frames(dev[:1], H, W, fmt)
    assert torch.equal(one, dev[:1]) and log1["psnr_y"] == float("inf")
    # 10 bits: the lumas are the codes over 1023
    fmt10 = FrameFormat("yuv420p", depth=10)
    host10 = ref.as_bytes(4 * noisy[:2] + 1, 10)
    l10 = TF.code_lumas(torch.from_numpy(host10).cuda(), H, W, fmt10).cpu().numpy()
    assert np.abs(l10.astype(np.float64) - (4 * noisy[:2, :H * W] + 1).reshape(2, H, W) / 1023.0).max() <= 2.0 ** -23


# ---- the C-ABI's refusals -----------------------------------------------------------------------------------------------------------
def test_abi_error_returns():
    L = _lib.lib()
    H, W, T = 16, 32, 18
    nb444 = frame_bytes(H, W, FrameFormat("yuv444p"))
    buf = torch.zeros((T, 2 * nb444 + 8), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((17, 2 * nb444 + 8), dtype=torch.uint8, device="cuda")
    flows = torch.zeros((17, 4, 2, H, W), dtype=torch.float32, device="cuda")
    sums = torch.zeros((17, 3), dtype=torch.int64, device="cuda")
    Y420, Y444, RGB = LAYOUTS["yuv420p"], LAYOUTS["yuv444p"], LAYOUTS["rgb24"]
    stride = int(buf.stride(0))
    lut = (C.c_uint16 * 64)(*LUT_B)
    bad_lut = (C.c_uint16 * 64)(*([257] + [0] * 63))

    def filt(T=T, first=0, n=1, H=H, W=W, layout=Y420, depth=8, q=(16, 16, 16), wt=(128, 64), lb=lut, lp=lut, src=buf.data_ptr(), sa=stride,
             out=dst.data_ptr(), so=stride, fl=flows.data_ptr()):
        rc = L.gsvc_tfilter_frames(src, sa, T, first, n, H, W, layout, depth, fl, (C.c_uint32 * 3)(*q) if q else None,
                                   (C.c_uint32 * 2)(*wt) if wt else None, lb, lp, out, so, None)
        return rc, L.gsvc_last_error().decode()

    def noise(n=1, H=H, W=W, layout=Y420, depth=8, src=buf.data_ptr(), sa=stride, o=sums.data_ptr()):
        rc = L.gsvc_noise_sums(src, sa, n, H, W, layout, depth, o, None)
        return rc, L.gsvc_last_error().decode()

    small = frame_bytes(H, W, FrameFormat("yuv420p")) - 1
    for call, text in ((filt(H=15), "even"), (filt(W=31), "even"), (filt(H=6), "at least 8"), (filt(n=17), "n must be"), (filt(n=0), "n must be"),
                       (filt(T=0), "T must be"), (filt(first=-1), "lie outside"), (filt(first=T - 1, n=2), "lie outside"), (filt(first=T), "lie outside"),
                       (filt(sa=small), "shorter than a frame"), (filt(so=small), "shorter than a frame"),
                       (filt(depth=10, sa=stride - 1), "multiple of 2"), (filt(depth=10, out=dst.data_ptr() + 1), "2-byte aligned"),
                       (filt(layout=RGB), "rgb24"), (filt(layout=7), "layout"), (filt(depth=9), "depth"), (filt(q=(0, 16, 16)), "q of plane 0"),
                       (filt(q=(16, 16, 65536)), "q of plane 2"), (filt(wt=(257, 0)), "wt[0]"), (filt(lb=bad_lut), "table entry"), (filt(lp=bad_lut), "table entry"),
                       (filt(q=None), "NULL"), (filt(lb=None), "NULL"), (filt(src=None), "NULL"), (filt(out=None), "NULL"), (filt(fl=None), "NULL"),
                       (filt(fl=flows.data_ptr() + 2), "4-byte aligned"), (filt(out=buf.data_ptr() + 3 * stride), "overlaps"),
                       (filt(src=dst.data_ptr(), T=4, out=dst.data_ptr() + 3 * stride + 16), "overlaps"),
                       (noise(H=15), "even"), (noise(W=6), "at least 8"), (noise(layout=RGB), "rgb24"), (noise(depth=11), "depth"), (noise(n=0), "n must be"),
                       (noise(n=17), "n must be"), (noise(sa=10), "shorter than a frame"), (noise(depth=16, sa=stride - 1, n=2), "multiple of 2"),
                       (noise(o=sums.data_ptr() + 4), "8-byte aligned"), (noise(src=None), "NULL"), (noise(o=None), "NULL")):
        assert call[0] == -1 and text in call[1], (call, text)
    torch.cuda.synchronize()
    assert not dst.any() and not sums.any()                                # nothing was launched
    sums.fill_(-1)
    assert filt(n=16, first=2, layout=Y444, depth=16)[0] == 0 and noise(n=16, layout=Y444, depth=16)[0] == 0
    torch.cuda.synchronize()
    assert not dst.any() and not sums[:16].any() and bool((sums[16] == -1).all())          # zero frames filter to zero; 16 rows were written
