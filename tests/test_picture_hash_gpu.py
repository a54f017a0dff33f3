"""GPU tests of the picture hash kernel (csrc/picture_hash.hip, ``metrics.picture_hash``): bit-equal to the NumPy statement of
tests/_picture_hash_ref.py for every layout and depth at the shapes where the kernel can go wrong — a frame smaller than a vector
(2 x 2), a plane that starts inside a 16-byte vector (6 x 10: H W = 60), the wide path with a tail (18 x 34), many narrow rows and more
than one workgroup per frame (1080 x 2), n = 1 and n = 3, a base moved by 2 bytes and an unaligned stride (the edge path), a slice of a
larger buffer whose other bytes are poisoned, two runs, and planes of the largest code (the width of the accumulators)."""
import numpy as np
import pytest
import torch

from gsvc_amd import frames_out as fo
from gsvc_amd import metrics
from gsvc_amd.frames_out import FrameFormat
from tests import _picture_hash_ref as ref

pytestmark = pytest.mark.gpu
FORMATS = [("rgb24", 8), ("yuv444p", 8), ("yuv420p", 8), ("yuv444p", 10), ("yuv420p", 10), ("yuv444p", 16), ("yuv420p", 16)]
SIZES = ((2, 2), (6, 10), (18, 34), (1080, 2))


def _random_frames(rng, n, H, W, fmt):
    nb = fo.frame_bytes(H, W, fmt)
    if fmt.depth == 8:
        return rng.integers(0, 256, (n, nb), dtype=np.uint8)
    return rng.integers(0, 1 << fmt.depth, (n, nb // 2), dtype=np.uint16).astype("<u2").view(np.uint8).reshape(n, nb)


def _placed(frames, stride, offset, guard):
    """The frames on the device in a buffer of ``guard`` bytes: frame k at offset + k * stride.  -> (the [n, stride] view, the buffer)."""
    n, nb = frames.shape
    buf = torch.full((offset + n * stride + 32,), guard, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + n * stride].view(n, stride)
    view[:, :nb] = torch.from_numpy(frames).cuda()
    return view, buf


def _bits(t):
    """int64 [n, 3] device tensor -> uint64 numpy."""
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("layout,depth", FORMATS, ids=[f"{l}-{d}" for l, d in FORMATS])
def test_picture_hash_is_the_reference_bit_for_bit(layout, depth):
    fmt = FrameFormat(layout, depth=depth)
    rng = np.random.default_rng(100 + depth + len(layout))
    for H, W in SIZES:
        nb = fo.frame_bytes(H, W, fmt)
        for n in (1, 3):
            a = _random_frames(rng, n, H, W, fmt)
            want = ref.picture_hash_ref(a, H, W, layout, depth)
            tight = metrics.picture_hash(torch.from_numpy(a).cuda(), H, W, fmt)
            assert tight.dtype == torch.int64 and tuple(tight.shape) == (n, 3)
            assert np.array_equal(_bits(tight), want), (H, W, n, "tight")
            # a stride above the frame, a multiple of 16: the wide path for n > 1 too
            stride = -(-nb // 16) * 16 + 16
            wide, _ = _placed(a, stride, 0, 0x5A)
            assert np.array_equal(_bits(metrics.picture_hash(wide, H, W, fmt)), want), (H, W, n, "stride")
            # the base moved by 2 bytes: the edge path
            moved, _ = _placed(a, stride, 2, 0xA5)
            assert np.array_equal(_bits(metrics.picture_hash(moved, H, W, fmt)), want), (H, W, n, "base + 2")
            # a stride that is no multiple of 16 (even, for the deep formats): the edge path for n > 1
            odd, _ = _placed(a, stride + 2, 0, 0x33)
            assert np.array_equal(_bits(metrics.picture_hash(odd, H, W, fmt)), want), (H, W, n, "stride + 2")


@pytest.mark.parametrize("layout,depth", [("rgb24", 8), ("yuv420p", 8), ("yuv420p", 10)])
@pytest.mark.parametrize("offset", [0, 2])
def test_nothing_outside_the_frames_is_read(layout, depth, offset):
    """Three frames inside a larger buffer: whatever the bytes before, between and behind them hold, the hashes are the same."""
    fmt = FrameFormat(layout, depth=depth)
    H, W = 18, 34
    nb = fo.frame_bytes(H, W, fmt)
    a = _random_frames(np.random.default_rng(9), 5, H, W, fmt)
    want = ref.picture_hash_ref(a[1:4], H, W, layout, depth)
    stride = -(-nb // 16) * 16 + 32
    view, buf = _placed(a, stride, offset, 0x00)
    first = metrics.picture_hash(view[1:4], H, W, fmt)
    assert np.array_equal(_bits(first), want)
    keep = view[1:4, :nb].clone()
    buf.fill_(0xFF)                                   # poison everything, then put the three frames back
    view[1:4, :nb] = keep
    assert torch.equal(metrics.picture_hash(view[1:4], H, W, fmt), first)
    tail = view[3]                                    # the last frame alone, as one flat frame: what follows it is poison
    assert torch.equal(metrics.picture_hash(tail[:nb], H, W, fmt), first[2:3])


def test_two_runs_give_the_same_bits():
    fmt = FrameFormat("yuv420p", depth=10)
    a = torch.from_numpy(_random_frames(np.random.default_rng(1), 3, 1080, 2, fmt)).cuda()
    assert torch.equal(metrics.picture_hash(a, 1080, 2, fmt), metrics.picture_hash(a, 1080, 2, fmt))


@pytest.mark.parametrize("layout,depth", FORMATS, ids=[f"{l}-{d}" for l, d in FORMATS])
def test_planes_of_the_largest_code(layout, depth):
    """Every code 2^d - 1 on 18 x 34 and 1080 x 2: the sums pass 2^32 (a 32-bit accumulator would wrap), the reference says what they are."""
    fmt = FrameFormat(layout, depth=depth)
    top = (1 << depth) - 1
    for H, W in ((18, 34), (1080, 2)):
        nb = fo.frame_bytes(H, W, fmt)
        if depth == 8:
            a = np.full((2, nb), top, np.uint8)
        else:
            a = np.full((2, nb // 2), top, np.uint16).astype("<u2").view(np.uint8).reshape(2, nb)
        want = ref.picture_hash_ref(a, H, W, layout, depth)
        assert int(want[0, 0]) > 2 ** 32
        assert np.array_equal(_bits(metrics.picture_hash(torch.from_numpy(a).cuda(), H, W, fmt)), want)
