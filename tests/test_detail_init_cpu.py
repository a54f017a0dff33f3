"""CPU tests of the content-adaptive initial anchors (gsvc_amd/detail.py, csrc/detail.hip): the NumPy / integer
statement of tests/_detail_ref.py on values done by hand, and everything of ``gsvc_frames_detail``, ``gsvc_detail_sample``, ``new_fit`` and the
two command-line tools that is decided before a device is needed."""
import os
import re
import sys

import numpy as np
import pytest

from gsvc_amd import _lib
from tests import _detail_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hash_known_answers():
    assert ref.hash_ref(0, 0, 0) == 0xE220A8397B1DCDAF
    assert ref.hash_ref(0, 0, 1) == 0x6E789E6AA1B965F4
    assert ref.hash_ref(1234, 7, 4) == 0x81FF459A9B93DB6A


def test_reference_map_by_hand():
    """Two frames of 3 x 3, cell 4 (one partial cell per frame).  Frame 0 = rows (1 2 4), (1 2 4), (7 2 4); frame 1 = frame 0 with the
    centre at 5.  By hand, frame 0: gx of rows 0 and 1 = |2-1| + |4-1| + |4-2| = 6, of row 2 = |2-7| + |4-7| + |4-2| = 10: 22; gy per column: column 0 = |1-1| + |7-1| + |7-1|
    = 12, columns 1 and 2 = 0; gt = |5 - 2| at the centre alone, counted twice: 6.  Sum 40.  Frame 1 looks back at frame 0: gx row 1 =
    |5-1| + |4-1| + |4-5| = 8 (rows 0 and 2: 6 and 10: 24); gy column 1 = |5-2| + |2-2| + |2-5| = 6, column 0 = 12: 18; gt 6.  Sum 48."""
    f0 = np.array([[1, 2, 4], [1, 2, 4], [7, 2, 4]])
    f1 = f0.copy()
    f1[1, 1] = 5
    m = ref.detail_map_ref(np.stack([f0, f1]), 4)
    assert m.shape == (2, 1, 1) and m[:, 0, 0].tolist() == [40, 48]
    assert ref.detail_map_ref(np.stack([f0, f1]), 4, n_out=1)[:, 0, 0].tolist() == [40]
    assert ref.detail_map_ref(f0[None], 4)[:, 0, 0].tolist() == [34]          # one frame: no temporal term
    # three frames: the middle one looks forward, the last one back
    f2 = f0.copy()
    f2[0, 0] = 3          # against f1: the corner (2) and the centre (3)
    m3 = ref.detail_map_ref(np.stack([f0, f1, f2]), 4)
    assert m3[1, 0, 0] == 42 + 2 * (2 + 3)          # f1's spatial terms: 24 + 18
    assert m3[2, 0, 0] == ref.detail_map_ref(f2[None], 4)[0, 0, 0] + 2 * (2 + 3)


def test_reference_map_cells_and_luma_view():
    """A 5 x 7 picture at cell 4 has 2 x 2 cells, the last row and column partial; the luma view takes the first H W samples as they are."""
    rng = np.random.default_rng(3)
    Y = rng.integers(0, 1024, (2, 5, 7))
    whole = ref.detail_map_ref(Y, 16)
    parts = ref.detail_map_ref(Y, 4)
    assert parts.shape == (2, 2, 2) and np.array_equal(parts.sum(axis=(1, 2)), whole[:, 0, 0])
    deep = np.zeros((2, 3 * 5 * 7 * 2 + 6), np.uint8)
    deep[:, :2 * 35] = Y.astype("<u2").reshape(2, 35).view(np.uint8)
    assert np.array_equal(ref.luma_of(deep, 5, 7, 10), Y)
    flat = rng.integers(0, 256, (2, 3 * 35), dtype=np.uint8)
    assert np.array_equal(ref.luma_of(flat, 5, 7, 8), flat[:, :35].reshape(2, 5, 7))


def test_upper_bound_skips_cells_of_weight_zero():
    m = np.array([[[0, 5, 0, 0], [0, 0, 7, 0]]])          # T = 1, 2 x 4 cells of 4 pixels: H = 8, W = 16
    pts, at = ref.sample_ref(m, 8, 16, 4, 2000, 0, 0)
    assert set(at.tolist()) == {1, 6}
    share = float(np.mean(at == 1))
    assert abs(share - 5 / 12) < 0.04          # (sigma = 0.011)
    in1, in6 = pts[at == 1], pts[at == 6]
    assert in1[:, 0].min() >= 4 and in1[:, 0].max() < 8 and in1[:, 1].min() >= 0 and in1[:, 1].max() < 4
    assert in6[:, 0].min() >= 8 and in6[:, 0].max() < 12 and in6[:, 1].min() >= 4 and in6[:, 1].max() < 8
    assert pts[:, 2].min() >= -0.5 and pts[:, 2].max() < 0.5
    # r = 0 takes the first cell of weight above zero, r = D - 1 the last one: never a neighbour of weight zero
    cdf = np.cumsum(m.reshape(-1))
    assert int(np.searchsorted(cdf, 0, side="right")) == 1 and int(np.searchsorted(cdf, 4, side="right")) == 1
    assert int(np.searchsorted(cdf, 5, side="right")) == 6 and int(np.searchsorted(cdf, 11, side="right")) == 6


def test_uniform_draws_and_the_mix():
    H, W, T, cell = 12, 20, 3, 8
    zero = np.zeros((T, 2, 3), np.int64)
    for m, mix24 in ((zero, 0), (np.ones_like(zero), 1 << 24)):          # D == 0, and mix = 1 on a map that has weight
        pts, at = ref.sample_ref(m, H, W, cell, 3000, 1234, mix24)
        x0, y0 = np.floor(pts[:, 0]).astype(int), np.floor(pts[:, 1]).astype(int)
        assert x0.min() == 0 and x0.max() == W - 1 and y0.min() == 0 and y0.max() == H - 1
        t = np.floor(pts[:, 2] + 0.5).astype(int)
        assert set(t.tolist()) == {0, 1, 2}
        assert np.array_equal(at, (t * 2 + y0 // cell) * 3 + x0 // cell)
        counts = np.bincount(t * H * W + y0 * W + x0, minlength=T * H * W)
        assert counts.max() <= 16          # 3000 draws over 720 pixels: a pixel, not a cell's corner, is what is drawn
    m = zero.copy()
    m[1, 1, 2], m[2, 0, 0] = 9, 1
    _, at = ref.sample_ref(m, H, W, cell, 3000, 0, 0)          # mix = 0: only the two cells of weight above zero
    assert set(at.tolist()) == {1 * 6 + 1 * 3 + 2, 2 * 6}
    _, at = ref.sample_ref(m, H, W, cell, 3000, 0, 1 << 22)          # mix = 0.25: the rest is spread
    assert 0.70 < np.mean(np.isin(at, [11, 12])) < 0.85 and len(set(at.tolist())) == 18


def test_placement_expectation_of_the_reference():
    """The placement clip at cell 8, mix 0.25, N = 4096, seed 0: the share of the points in the top-left quadrant is 0.75 + 0.25 / 4 =
    0.8125 in expectation; the reference's draw gives 0.807."""
    H, W = 48, 64
    frames = ref.quadrant_clip()
    m = ref.detail_map_ref(ref.luma_of(frames, H, W, 8), 8)
    assert m[:, 3:, :].sum() == 0 and m[:, :, 4:].sum() == 0 and m.sum() > 0
    pts, _ = ref.sample_ref(m, H, W, 8, 4096, 0, 1 << 22)
    share = float(np.mean((pts[:, 0] < W / 2) & (pts[:, 1] < H / 2)))
    assert 0.78 <= share and abs(share - 0.807) < 0.0006, share


def test_new_symbols_in_header_and_binding():
    text = open(os.path.join(ROOT, "include", "gsvc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("gsvc_frames_detail", "gsvc_detail_sample"):
        assert re.search(rf"\bint {name}\s*\(", code), name
        assert name in _lib.declared_symbols()
        assert hasattr(_lib.lib(), name)
    assert "init_point_cloud" in text and "init_point_cloud" in open(os.path.join(ROOT, "gsvc_amd", "detail.py")).read()


def test_frames_detail_entry_point_validates_on_the_host():
    L = _lib.lib()
    ok = (64, 48, 2, 2, 4, 4, 2, 8, 8, 256, None)          # frames, stride, n, n_out, H, W, layout, depth, cell, out, stream
    def put(i, v):
        return ok[:i] + (v,) + ok[i + 1:]
    cases = [(put(0, None), b"NULL"), (put(9, None), b"NULL"), (put(6, 0), b"rgb24"), (put(6, 3), b"unknown layout"),
             (put(7, 9), b"depth must be 8, 10, 12 or 16"), (put(7, 14), b"depth must be 8, 10, 12 or 16"), (put(7, 7), b"depth must be"),
             (put(7, 17), b"depth must be"), (put(8, 5), b"cell must be 4, 8 or 16"), (put(8, 32), b"cell must be"), (put(8, 0), b"cell must be"),
             (put(3, 3), b"n_out must be"), (put(3, 0), b"n_out must be"), (put(2, 0), b"n must be"), (put(2, 65536), b"n must be"),
             (put(1, 23), b"shorter than a frame"), (put(4, 3), b"even"), (put(4, 0), b"image size"),
             ((65, 96, 2, 2, 4, 4, 1, 10, 8, 256, None), b"2-byte aligned"), ((64, 97, 2, 2, 4, 4, 1, 10, 8, 256, None), b"multiple of 2"),
             (put(9, 258), b"4-byte aligned")]
    for args, msg in cases:
        assert L.gsvc_frames_detail(*args) == -1, args
        err = L.gsvc_last_error()
        assert msg in err and err.startswith(b"frames_detail:"), (args, err)


def test_detail_sample_entry_point_validates_on_the_host():
    L = _lib.lib()
    ok = (64, 2 * 6 * 8, 2, 48, 64, 8, 100, 0, 1 << 22, 4096, 8192, None)   # cdf, cells, T, H, W, cell, N, seed, mix24, points, cell_of, stream
    def put(i, v):
        return ok[:i] + (v,) + ok[i + 1:]
    cases = [(put(0, None), b"NULL"), (put(9, None), b"NULL"), (put(10, None), b"NULL"), (put(1, 95), b"cells must be"),
             (put(3, 50), b"cells must be"), (put(5, 16), b"cells must be"), (put(8, (1 << 24) + 1), b"mix24 must be"), (put(5, 5), b"cell must be"),
             (put(6, 0), b"N must be"), (put(2, 0), b"T must be"), (put(4, 0), b"image size"), (put(0, 68), b"aligned"),
             ((64, 65535 * 2048 * 2048, 65535, 8192, 8192, 4, 100, 0, 0, 4096, 8192, None), b"too large")]
    for args, msg in cases:
        assert L.gsvc_detail_sample(*args) == -1, args
        err = L.gsvc_last_error()
        assert msg in err and err.startswith(b"detail_sample:"), (args, err)


def test_python_layer_refuses_before_a_device_is_needed():
    import torch

    from gsvc_amd import detail
    from gsvc_amd.fit_setup import new_fit
    from gsvc_amd.frames_out import FrameFormat
    with pytest.raises(ValueError, match=r"init must be one of uniform, detail.*'nonsense'"):
        new_fit(None, None, None, None, 100, "cpu", init="nonsense")
    with pytest.raises(ValueError, match="cell must be one of 4, 8, 16"):
        new_fit(None, None, None, None, 100, "cpu", init="detail", init_cell=5)
    with pytest.raises(ValueError, match=r"mix must lie in \[0, 1\]"):
        new_fit(None, None, None, None, 100, "cpu", init="detail", init_mix=1.5)
    a = torch.zeros((2, 24), dtype=torch.uint8)
    with pytest.raises(ValueError, match="rgb24 frames hold no luma plane"):
        detail.luma_detail(torch.zeros((2, 48), dtype=torch.uint8), 4, 4, FrameFormat("rgb24"))
    with pytest.raises(_lib.GsvcError, match="CPU tensors are not supported"):
        detail.luma_detail(a, 4, 4, FrameFormat("yuv420p"))
    with pytest.raises(ValueError, match="cell must be one of"):
        detail.luma_detail(a, 4, 4, FrameFormat("yuv420p"), cell=3)
    assert detail.mix24_of(0.0) == 0 and detail.mix24_of(0.25) == 1 << 22 and detail.mix24_of(1.0) == 1 << 24
    assert detail.map_shape(50, 70, 8) == (7, 9) and detail.map_shape(48, 64, 16) == (3, 4)


def test_chunks_overlap_by_one_frame_and_the_last_one_looks_back():
    from gsvc_amd.detail import CHUNK, chunks
    assert CHUNK == 16
    assert chunks(1) == [(0, 1, 1)] and chunks(2) == [(0, 2, 2)] and chunks(16) == [(0, 16, 16)] and chunks(17) == [(0, 17, 17)]
    assert chunks(18) == [(0, 17, 16), (16, 2, 2)] and chunks(33) == [(0, 17, 16), (16, 17, 17)] and chunks(34) == [(0, 17, 16), (16, 17, 16), (32, 2, 2)]
    for T in range(1, 70):
        plan = chunks(T)
        assert [s for s, _, _ in plan] == [16 * k for k in range(len(plan))] and sum(o for _, _, o in plan) == T
        assert all(n == 17 and o == 16 for _, n, o in plan[:-1]) and plan[-1][0] + plan[-1][1] == T and (T == 1 or plan[-1][1] >= 2)


@pytest.mark.parametrize("tool", ["gsvc_encode", "fit_synthetic"])
def test_tools_refuse_init_mix_without_init_detail(tool, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    mod = __import__(tool)
    base = ["clip.y4m", "-o", "clip.gsvc"] if tool == "gsvc_encode" else []
    for extra in (["--init-mix", "0.5"], ["--init", "uniform", "--init-mix", "0.5"], ["--init-cell", "4"], ["--init", "detail", "--init-mix", "1.5"],
                  ["--init", "detail", "--init-cell", "5"], ["--init", "sobel"]):
        with pytest.raises(SystemExit) as e:
            mod.main(base + extra)
        assert e.value.code == 2, extra
    assert "need --init detail" in capsys.readouterr().err
