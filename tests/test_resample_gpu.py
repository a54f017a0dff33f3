"""GPU tests of the resampler kernel (csrc/resample.hip): ``resample_frames`` and the raw C-ABI bit-equal to
tests/_resample_ref.py on both layouts and depths 8, 10 and 16, with padded strides and guard bytes; batches; poisoned table slots; the
ABI's refusals.  Sizes are written W x H; the kernel's tile is 64 x 16 output samples."""
import os
import sys

import numpy as np
import pytest
import torch

from gsvc_amd import _lib
from gsvc_amd import resample as R
from gsvc_amd.frames_out import LAYOUTS, FrameFormat, frame_bytes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resample_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 0xA5
PAD = 6                     # bytes behind every frame of a padded buffer (even: deep formats)
#        from        to
SIZES = (((16, 24), (8, 12)),
         ((16, 24), (32, 48)),
         ((38, 70), (26, 46)),
         ((38, 70), (54, 30)),          # up in one axis, down in the other
         ((8, 8), (2, 2)),              # 24 taps over 8 samples; 4:2:0 chroma 4 -> 1, every tap clamped
         ((2, 2), (8, 8)),              # chroma 1 x 1
         ((40, 40), (10, 160)),
         ((64, 96), (64, 96)),          # output bytes equal the input
         ((258, 66), (130, 34)))        # just over two tiles of output in each axis
_TAPS = {}


def taps(src, dst):
    if (src, dst) not in _TAPS:
        _TAPS[(src, dst)] = R.filter_taps(src, dst)
    return _TAPS[(src, dst)]


def make_frames(H, W, fmt, seed=0):
    """Three frames: full-range noise (for a deep format every 16-bit word, also above the format's peak: codes are read as they are),
    the 0 / peak checkerboard on every plane, constant peak."""
    nb = frame_bytes(H, W, fmt)
    rng = np.random.default_rng(seed)
    peak = (1 << fmt.depth) - 1
    noise = rng.integers(0, 256, nb, dtype=np.uint8)
    planes = []
    for h, w in ref.plane_dims(H, W, fmt.layout):
        planes.append((((np.arange(h)[:, None] + np.arange(w)[None]) & 1) * peak).reshape(-1))
    checker = np.concatenate(planes)
    const = np.full_like(checker, peak)
    as_bytes = (lambda a: a.astype("<u2").view(np.uint8)) if fmt.depth > 8 else (lambda a: a.astype(np.uint8))
    return np.stack([noise, as_bytes(checker), as_bytes(const)])


def padded(frames, pad=PAD):
    """The frames in a device buffer whose rows are ``pad`` guard bytes longer."""
    n, nb = frames.shape
    buf = torch.full((n, nb + pad), GUARD, dtype=torch.uint8, device="cuda")
    buf[:, :nb] = torch.from_numpy(frames).cuda()
    return buf


@pytest.mark.parametrize("depth", (8, 10, 16))
@pytest.mark.parametrize("layout", ("yuv420p", "yuv444p"))
def test_kernel_is_bit_equal_to_the_reference(layout, depth):
    fmt = FrameFormat(layout, depth=depth)
    for (W, H), (oW, oH) in SIZES:
        frames = make_frames(H, W, fmt, seed=W + oW)
        want = ref.resample_frames(frames, H, W, layout, depth, oH, oW, taps)
        ob = frame_bytes(oH, oW, fmt)
        src = padded(frames)
        out = torch.full((3, ob + PAD), GUARD, dtype=torch.uint8, device="cuda")
        got = R.resample_frames(src, H, W, fmt, oH, oW, out=out)
        assert got.shape == (3, ob) and got.data_ptr() == out.data_ptr()
        host = out.cpu().numpy()
        assert np.array_equal(host[:, :ob], want), (layout, depth, (W, H), (oW, oH))
        assert (host[:, ob:] == GUARD).all() and (src.cpu().numpy()[:, -PAD:] == GUARD).all()          # guard bytes untouched
        fresh = R.resample_frames(src[:, :frame_bytes(H, W, fmt)], H, W, fmt, oH, oW)                   # (a buffer of its own, no padding on the output)
        assert np.array_equal(fresh.cpu().numpy(), want)
        if (W, H) == (oW, oH):          # the input bytes (a word above the peak of a 10-bit frame comes back as the peak: the final clamp)
            same = np.minimum(frames.view("<u2"), (1 << depth) - 1).view(np.uint8) if depth > 8 else frames
            assert np.array_equal(want, same) and np.array_equal(want[1:], frames[1:])
    one = R.resample_frames(torch.from_numpy(make_frames(24, 16, fmt)[0]).cuda(), 24, 16, fmt, 12, 8)          # one flat frame
    assert one.shape == (1, frame_bytes(12, 8, fmt))
    assert np.array_equal(one.cpu().numpy(), ref.resample_frames(make_frames(24, 16, fmt)[:1], 24, 16, layout, depth, 12, 8, taps))


def test_batches_equal_single_calls():
    fmt = FrameFormat("yuv420p", depth=10)
    (W, H), (oW, oH) = (38, 70), (26, 46)
    nb = frame_bytes(H, W, fmt)
    frames = np.random.default_rng(5).integers(0, 256, (17, nb), dtype=np.uint8)
    frames.view("<u2")[:] &= 1023
    dev = torch.from_numpy(frames).cuda()
    singles = torch.cat([R.resample_frames(dev[k], H, W, fmt, oH, oW) for k in range(17)]).cpu().numpy()
    assert np.array_equal(singles[:3], ref.resample_frames(frames[:3], H, W, "yuv420p", 10, oH, oW, taps))
    for n in (1, 3, 17):
        assert np.array_equal(R.resample_frames(dev[:n], H, W, fmt, oH, oW).cpu().numpy(), singles[:n]), n


def _abi_tables(W, H, oW, oH, layout, poison=False):
    """The twelve table arguments of the ABI as fresh device arrays (kept alive by the list returned with them)."""
    sub = layout == "yuv420p"
    cw, ch, ocw, och = (W // 2, H // 2, oW // 2, oH // 2) if sub else (W, H, oW, oH)
    keep, args = [], []
    for s, d in ((W, oW), (H, oH), (cw, ocw), (ch, och)):
        first, coef, nt = taps(s, d)
        coef = coef.copy()
        if poison:
            coef[:, nt:] = 0x7FFF
        first_d, coef_d = torch.from_numpy(first).cuda(), torch.from_numpy(coef).cuda()
        keep += [first_d, coef_d]
        args += [first_d.data_ptr(), coef_d.data_ptr(), nt]
    return args, keep


@pytest.mark.parametrize("layout,depth", (("yuv420p", 8), ("yuv444p", 16)))
def test_raw_abi_and_poisoned_slots_behind_nt(layout, depth):
    fmt = FrameFormat(layout, depth=depth)
    L = _lib.lib()
    for (W, H), (oW, oH) in (((38, 70), (54, 30)), ((16, 24), (32, 48)), ((258, 66), (130, 34))):
        frames = make_frames(H, W, fmt, seed=3)
        want = ref.resample_frames(frames, H, W, layout, depth, oH, oW, taps)
        src, ob = padded(frames), frame_bytes(oH, oW, fmt)
        for poison in (False, True):
            args, keep = _abi_tables(W, H, oW, oH, layout, poison)
            assert min(args[2::3]) < 24                   # (there are slots to poison)
            out = torch.full((3, ob + PAD), GUARD, dtype=torch.uint8, device="cuda")
            rc = L.gsvc_resample_frames(src.data_ptr(), src.stride(0), 3, H, W, LAYOUTS[layout], depth, out.data_ptr(), out.stride(0), oH, oW,
                                        *args, None)
            assert rc == 0, L.gsvc_last_error().decode()
            host = out.cpu().numpy()
            assert np.array_equal(host[:, :ob], want) and (host[:, ob:] == GUARD).all(), (layout, depth, W, H, poison)
            del keep


def test_abi_refusals():
    L = _lib.lib()
    Y444, Y420, RGB = LAYOUTS["yuv444p"], LAYOUTS["yuv420p"], LAYOUTS["rgb24"]
    H, W, oH, oW = 24, 16, 12, 8
    stride, ostride = 2 * 3 * H * W + 16, 2 * 3 * oH * oW + 16
    buf = torch.zeros((16, stride), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((16, ostride), dtype=torch.uint8, device="cuda")
    tab, keep = _abi_tables(W, H, oW, oH, "yuv444p")

    def call(n=1, H=H, W=W, layout=Y420, depth=8, src=buf.data_ptr(), sa=stride, out=dst.data_ptr(), so=ostride, oH=oH, oW=oW, t=None):
        rc = L.gsvc_resample_frames(src, sa, n, H, W, layout, depth, out, so, oH, oW, *(tab if t is None else t), None)
        return rc, L.gsvc_last_error().decode()

    def tables(**kw):
        t = list(tab)
        for k, v in kw.items():
            t[int(k[1:])] = v
        return t

    small_in, small_out = frame_bytes(H, W, FrameFormat("yuv420p")) - 1, frame_bytes(oH, oW, FrameFormat("yuv420p")) - 1
    for got, text in ((call(src=None), "NULL"), (call(out=None), "NULL"), (call(t=tables(a0=None)), "NULL"), (call(t=tables(a10=None)), "NULL"),
                      (call(layout=RGB), "rgb24"), (call(layout=7), "layout"), (call(depth=9), "depth"), (call(depth=14), "depth"),
                      (call(n=0), "n must be"), (call(n=17), "n must be"), (call(H=23), "even"), (call(oW=7), "even"), (call(oH=11), "even"),
                      (call(layout=Y444, W=1), "at least 2"), (call(layout=Y444, oH=1), "at least 2"),
                      (call(oW=2), "ratio of 4"), (call(layout=Y444, H=49), "ratio of 4"), (call(W=4, oW=18), "ratio of 4"),
                      (call(t=tables(a2=0)), "nt must be"), (call(t=tables(a5=25)), "nt must be"), (call(t=tables(a11=-1)), "nt must be"),
                      (call(sa=small_in), "shorter than a frame"), (call(so=small_out), "shorter than a frame"),
                      (call(depth=10, sa=stride - 1, n=2), "multiple of 2"), (call(depth=16, so=ostride - 1, n=2), "multiple of 2"),
                      (call(depth=10, src=buf.data_ptr() + 1), "2-byte aligned"), (call(depth=12, out=dst.data_ptr() + 1), "2-byte aligned"),
                      (call(t=tables(a0=tab[0] + 2)), "aligned"), (call(t=tables(a4=tab[4] + 1)), "aligned"),
                      (call(out=buf.data_ptr() + 64), "overlaps"), (call(n=4, src=dst.data_ptr() + 2 * ostride, sa=small_in + 1), "overlaps")):
        assert got[0] == -1 and text in got[1], (got, text)
    torch.cuda.synchronize()
    assert not dst.any()                                   # nothing was launched
    buf.fill_(200)
    assert call(n=16, layout=Y444, depth=8)[0] == 0
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    assert (host[:, :3 * oH * oW] == 200).all() and not host[:, 3 * oH * oW:].any()          # a constant stays constant; bytes behind the frames untouched
    del keep
    with pytest.raises(ValueError, match="out must hold"):
        R.resample_frames(buf[:2, :3 * H * W], H, W, FrameFormat("yuv444p"), oH, oW, out=dst[:3])
    with pytest.raises(_lib.GsvcError):
        R.resample_frames(buf[:1, :3 * H * W].cpu(), H, W, FrameFormat("yuv444p"), oH, oW)
