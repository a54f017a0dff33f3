"""The frame kernels reproduce, bit for bit, what the library of an earlier commit gave: the digests of tests/_frames_bits.py against
tests/golden/frames_bits.json (recorded with the commit the file names, through GSVC_LIB_PATH; see the helper).  Every output byte of
csrc/frames_out.hip, every float of csrc/frames_in.hip and every sum of k_frames_sse / k_picture_hash on the helper's seeded inputs —
all layouts, depths 8 / 10 / 16, matrices, ranges, roundings and chroma modes, the wide and the edge path of every kernel."""
import pytest

from tests import _frames_bits as bits

pytestmark = pytest.mark.gpu
IDS = [f"{layout}-{depth}" for layout, depth in bits.FORMATS]


def _compare(got, prefix):
    want = {k: v for k, v in bits.golden()["digests"].items() if k.startswith(prefix)}
    assert sorted(got) == sorted(want)          # the recorded cases are the cases of today's helper
    differing = [k for k in sorted(got) if got[k] != want[k]]
    assert not differing, differing


@pytest.mark.parametrize("layout,depth", bits.FORMATS, ids=IDS)
def test_output_bytes_are_those_of_the_recorded_build(layout, depth):
    _compare(bits.out_digests(layout, depth), f"out/{layout}/{depth}/")


@pytest.mark.parametrize("layout,depth", bits.FORMATS, ids=IDS)
def test_input_floats_are_those_of_the_recorded_build(layout, depth):
    _compare(bits.in_digests(layout, depth), f"in/{layout}/{depth}/")


@pytest.mark.parametrize("layout,depth", bits.FORMATS, ids=IDS)
def test_sse_and_hash_sums_are_those_of_the_recorded_build(layout, depth):
    got = bits.sums_digests(layout, depth)
    _compare({k: v for k, v in got.items() if k.startswith("sse/")}, f"sse/{layout}/{depth}/")
    _compare({k: v for k, v in got.items() if k.startswith("hash/")}, f"hash/{layout}/{depth}/")
