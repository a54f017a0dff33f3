"""GPU tests of the histogram kernel (csrc/scene.hip, ``metrics.plane_histograms``): bit-equal to the NumPy statement of
tests/_scene_ref.py for every layout at depths 8, 10 and 16 at the shapes of the picture-hash test — a frame smaller than a vector
(2 x 2), a plane that starts inside a 16-byte vector (6 x 10: H W = 60), the wide path with a tail (18 x 34), many narrow rows (1080 x 2)
— and at 96 x 64 and 160 x 300 (more than one workgroup per frame: a workgroup walks 2 048 samples on the edge path and 2 048
16-byte units on the wide path; a 160 x 300 4:2:0 frame has 4 500 units of 8-bit samples), n = 1 and n = 3, a base
moved by 1 byte (8-bit) or 2 bytes (deep) and a stride that is no multiple of 16 (the edge path), surroundings poisoned with 0xFF, and
three contents: seeded noise, a constant frame (every lane on one counter) and a ramp in which every bin is present."""
import numpy as np
import pytest
import torch

from gsvc_amd import frames_out as fo
from gsvc_amd import metrics
from gsvc_amd.frames_out import FrameFormat
from tests import _scene_ref as ref

pytestmark = pytest.mark.gpu
FORMATS = [("rgb24", 8), ("yuv444p", 8), ("yuv420p", 8), ("yuv444p", 10), ("yuv420p", 10), ("yuv444p", 16), ("yuv420p", 16)]
SIZES = ((2, 2), (6, 10), (18, 34), (1080, 2), (96, 64), (160, 300))


def _codes(a, fmt, n, nb):
    """uint8 / uint16 codes [n, samples] -> the frames' bytes, uint8 [n, nb]."""
    if fmt.depth == 8:
        return np.ascontiguousarray(a.astype(np.uint8))
    return a.astype("<u2").view(np.uint8).reshape(n, nb)


def _frames(content, rng, n, H, W, fmt):
    nb = fo.frame_bytes(H, W, fmt)
    samples = nb // (2 if fmt.depth > 8 else 1)
    if content == "noise":
        a = rng.integers(0, 1 << fmt.depth, (n, samples))
    elif content == "constant":
        a = np.full((n, samples), (1 << fmt.depth) * 5 // 8 + 3)
    else:                                             # every bin present: a ramp through all codes' upper eight bits, frame k shifted by k
        a = ((np.arange(samples)[None, :] + np.arange(n)[:, None]) % 256) << (fmt.depth - 8)
    return _codes(a, fmt, n, nb)


def _placed(frames, stride, offset):
    """The frames on the device in a buffer of 0xFF bytes: frame k at offset + k * stride.  -> the [n, stride] view (it keeps the buffer)."""
    n, nb = frames.shape
    buf = torch.full((offset + n * stride + 32,), 0xFF, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + n * stride].view(n, stride)
    view[:, :nb] = torch.from_numpy(frames).cuda()
    return view


def _check(got, want, what):
    assert got.dtype == torch.int32 and tuple(got.shape) == want.shape, what
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want), what


@pytest.mark.parametrize("content", ["noise", "constant", "every_bin"])
@pytest.mark.parametrize("layout,depth", FORMATS, ids=[f"{l}-{d}" for l, d in FORMATS])
def test_histograms_are_the_reference_bit_for_bit(layout, depth, content):
    fmt = FrameFormat(layout, depth=depth)
    rng = np.random.default_rng(200 + depth + len(layout))
    step = 1 if depth == 8 else 2
    for H, W in SIZES:
        nb = fo.frame_bytes(H, W, fmt)
        counts = metrics.plane_samples(H, W, fmt)
        for n in (1, 3):
            a = _frames(content, rng, n, H, W, fmt)
            want = ref.histogram_ref(a, H, W, layout, depth)
            assert want.sum(axis=2).tolist() == [list(counts)] * n
            if content == "every_bin" and H * W >= 1024:
                assert (want[:, 0] > 0).all()
            tight = metrics.plane_histograms(torch.from_numpy(a).cuda(), H, W, fmt)
            _check(tight, want, (H, W, n, "tight"))
            assert tight.sum(dim=2).tolist() == [list(counts)] * n          # per plane, the bins sum to the plane's samples
            stride = -(-nb // 16) * 16 + 16                                  # a stride above the frame, a multiple of 16: the wide path
            _check(metrics.plane_histograms(_placed(a, stride, 0), H, W, fmt), want, (H, W, n, "stride"))
            _check(metrics.plane_histograms(_placed(a, stride, step), H, W, fmt), want, (H, W, n, "base moved"))
            _check(metrics.plane_histograms(_placed(a, stride + step, 0), H, W, fmt), want, (H, W, n, "stride no multiple of 16"))
            _check(metrics.plane_histograms(_placed(a, stride + step, 16 + step), H, W, fmt), want, (H, W, n, "both"))


def test_stray_upper_bits_of_a_deep_sample_count_in_the_last_bin():
    """A 10-bit frame holding 0xFFFF samples: 0xFFFF >> 2 is far above 255, the min keeps it inside the plane's counters — the samples
    land in bin 255 of THEIR plane and nowhere else."""
    fmt = FrameFormat("yuv420p", depth=10)
    for H, W in ((6, 10), (18, 34)):
        nb = fo.frame_bytes(H, W, fmt)
        a = np.full((2, nb // 2), 0xFFFF, np.uint16)
        a[1, ::3] = 512
        a = _codes(a, fmt, 2, nb)
        want = ref.histogram_ref(a, H, W, "yuv420p", 10)
        counts = metrics.plane_samples(H, W, fmt)
        assert want[0, :, 255].tolist() == list(counts) and want[0].sum() == sum(counts) and want[1, 0, 128] > 0
        for view in (torch.from_numpy(a).cuda(), _placed(a, nb + 2, 2)):
            _check(metrics.plane_histograms(view, H, W, fmt), want, (H, W))


def test_two_calls_give_equal_bits_and_the_output_is_zeroed_by_the_call():
    fmt = FrameFormat("yuv420p", depth=10)
    a = torch.from_numpy(_frames("noise", np.random.default_rng(1), 3, 1080, 2, fmt)).cuda()
    first = metrics.plane_histograms(a, 1080, 2, fmt)
    for _ in range(3):                                # (the allocator hands the same memory out again: counts of the call before are gone)
        again = metrics.plane_histograms(a, 1080, 2, fmt)
        assert torch.equal(again, first)
        del again


def test_a_slice_of_a_larger_buffer():
    """Three frames inside a buffer of five: the other two, and everything between and behind, change nothing."""
    fmt = FrameFormat("yuv420p")
    H, W = 18, 34
    nb = fo.frame_bytes(H, W, fmt)
    a = _frames("noise", np.random.default_rng(9), 5, H, W, fmt)
    want = ref.histogram_ref(a[1:4], H, W, "yuv420p", 8)
    for offset in (0, 1):
        view = _placed(a, -(-nb // 16) * 16 + 32, offset)
        _check(metrics.plane_histograms(view[1:4], H, W, fmt), want, offset)
        view[0].fill_(0xFF)
        view[4].fill_(0xFF)
        _check(metrics.plane_histograms(view[1:4], H, W, fmt), want, offset)
        _check(metrics.plane_histograms(view[3][:nb], H, W, fmt), want[2:3], offset)
