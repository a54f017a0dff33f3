"""CPU tests of the deep (10 / 12 / 16-bit) frame formats: the float64 reference of tests/_frames_hbd_ref.py on values that can be
checked by hand and against the two 8-bit references at depth 8, the Python side of gsvc_amd/frames_out.py and frames_in.py
(``FrameFormat(depth=...)``, ``frame_bytes``, ``planes``, Y4M headers, ``read_y4m``, ``open_video``) and the host-side refusals of
gsvc_frames_bytes / gsvc_frames_to_u16 / gsvc_frames_from_u16.  No GPU is used."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from gsvc_amd import _lib
from gsvc_amd import frames_in as fi
from gsvc_amd import frames_out as fo
from gsvc_amd.frames_out import FrameFormat
from tests import _frames_hbd_ref as ref
from tests import _frames_in_ref as ref_in8
from tests import _frames_ref as ref_out8

COMBOS = [(m, r) for m in ("bt709", "bt601") for r in ("limited", "full")]


# ---- the reference on hand-checkable values ---------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
def test_black_white_and_grey_codes_at_10_bits(matrix):
    black, white, grey = (np.full((3, 1, 1), v) for v in (0.0, 1.0, 0.5))
    assert list(ref.convert(black, "yuv444p", matrix, "limited", "nearest", 10)) == [64, 512, 512]
    assert list(ref.convert(white, "yuv444p", matrix, "limited", "nearest", 10)) == [940, 512, 512]
    assert list(ref.convert(black, "yuv444p", matrix, "full", "nearest", 10)) == [0, 512, 512]
    assert list(ref.convert(white, "yuv444p", matrix, "full", "nearest", 10)) == [1023, 512, 512]
    assert list(ref.convert(grey, "yuv444p", matrix, "limited", "nearest", 10)) == [502, 512, 512]          # 64 + 876 / 2
    assert ref.convert(grey, "yuv444p", matrix, "full", "trunc", 10)[0] == 511                              # 1023 / 2 = 511.5
    # and back: the codes 64 / 940 / 512 and 0 / 1023 / 512
    assert np.array_equal(ref.rgb_of_codes(64, 512, 512, matrix, "limited", 10), [0.0, 0.0, 0.0])
    assert np.array_equal(ref.rgb_of_codes(940, 512, 512, matrix, "limited", 10), [1.0, 1.0, 1.0])
    assert np.allclose(ref.rgb_of_codes(512, 512, 512, matrix, "limited", 10), 448.0 / 876.0, rtol=0, atol=1e-15)
    assert np.array_equal(ref.rgb_of_codes(0, 512, 512, matrix, "full", 10), [0.0, 0.0, 0.0])
    assert np.array_equal(ref.rgb_of_codes(1023, 512, 512, matrix, "full", 10), [1.0, 1.0, 1.0])
    assert np.allclose(ref.rgb_of_codes(512, 512, 512, matrix, "full", 10), 512.0 / 1023.0, rtol=0, atol=1e-15)
    assert np.array_equal(ref.rgb_of_codes(1023, 512, 512, matrix, "limited", 10), [1.0, 1.0, 1.0])          # above white: clamped


@pytest.mark.parametrize("depth", [10, 12, 16])
def test_constants_scale_with_the_depth(depth):
    up = 2 ** (depth - 8)
    assert ref.constants(depth, "limited") == (16 * up, 219 * up, 2 ** (depth - 1), 224 * up, 2 ** depth - 1)
    assert ref.constants(depth, "full") == (0, 2 ** depth - 1, 2 ** (depth - 1), 2 ** depth - 1, 2 ** depth - 1)
    # a red pixel, by hand, BT.601 full range: Y = 0.299, Cr = 0.5, Cb = -0.299 * ... / 1.772
    red = np.array([1.0, 0.0, 0.0]).reshape(3, 1, 1)
    top = 2 ** depth - 1
    v = ref.values(red, "yuv444p", "bt601", "full", depth)
    assert np.allclose(v, [0.299 * top, 2 ** (depth - 1) + top * (0.0 - 0.299) / 1.772, min(top, 2 ** (depth - 1) + top * 0.5)], rtol=0, atol=1e-9)


def test_chroma_edge_upsampling_weights():
    """One vertical chroma edge, c = [[0, 1000], [0, 1000]] -> 4 x 4: the columns are 0, 250, 750, 1000 in every row; and one
    horizontal edge likewise.  A single interior sample spreads as 9/16, 3/16, 3/16, 1/16."""
    up = ref.upsample_codes([[0, 1000], [0, 1000]], "bilinear")
    assert np.array_equal(up, np.tile([0.0, 250.0, 750.0, 1000.0], (4, 1)))
    assert np.array_equal(ref.upsample_codes([[0, 0], [1000, 1000]], "bilinear"), np.tile([0.0, 250.0, 750.0, 1000.0], (4, 1)).T)
    c = np.zeros((3, 3))
    c[1, 1] = 1600
    want = np.array([[0, 0, 0, 0, 0, 0], [0, 100, 300, 300, 100, 0], [0, 300, 900, 900, 300, 0],
                     [0, 300, 900, 900, 300, 0], [0, 100, 300, 300, 100, 0], [0, 0, 0, 0, 0, 0]], dtype=np.float64)
    assert np.array_equal(ref.upsample_codes(c, "bilinear"), want)
    assert np.array_equal(ref.upsample_codes([[1, 2], [3, 4]], "nearest"), [[1, 1, 2, 2], [1, 1, 2, 2], [3, 3, 4, 4], [3, 3, 4, 4]])
    # a frame through it: a 2 x 4 yuv420p frame at 10 bits, full range, luma 0, U = [100, 900], V = 512: B rises along the row
    codes = np.array([0] * 8 + [100, 900] + [512, 512])
    img = ref.image(codes, 2, 4, "yuv420p", "bt709", "full", "bilinear", 10)
    cb = (np.array([100.0, 300.0, 700.0, 900.0]) - 512.0) / 1023.0
    assert np.allclose(img[2], np.clip(1.8556 * cb, 0, 1)[None, :].repeat(2, 0), rtol=0, atol=1e-15)


@pytest.mark.parametrize("matrix,rng", COMBOS)
def test_depth_8_reproduces_the_8_bit_references(matrix, rng):
    for layout in ("yuv444p", "yuv420p"):
        for kind in ref_out8.KINDS:
            img = ref_out8.make_image(kind, 18, 50, seed=3)
            assert np.array_equal(ref.values(img, layout, matrix, rng, 8), ref_out8.values(img, layout, matrix, rng))
            for rounding in ("trunc", "nearest"):
                assert np.array_equal(ref.convert(img, layout, matrix, rng, rounding, 8), ref_out8.convert(img, layout, matrix, rng, rounding))
        for chroma in ("bilinear", "nearest"):
            frame = ref_in8.random_frame(18, 50, layout, 4)
            assert np.array_equal(ref.image(ref.from_bytes(frame, 8), 18, 50, layout, matrix, rng, chroma, 8),
                                  ref_in8.values(frame, 18, 50, layout, matrix, rng, chroma))
    frame = ref_in8.checkerboard_frame(16, 32, 5)
    assert np.array_equal(ref.image(ref.from_bytes(frame, 8), 16, 32, "yuv420p", matrix, rng, "bilinear", 8),
                          ref_in8.values(frame, 16, 32, "yuv420p", matrix, rng, "bilinear"))


def test_bytes_of_codes_are_little_endian_words():
    assert list(ref.to_bytes([0x0123, 0x03FF], 10)) == [0x23, 0x01, 0xFF, 0x03]
    assert list(ref.from_bytes([0x23, 0x01, 0xFF, 0x03], 10)) == [0x0123, 0x03FF]
    assert list(ref.to_bytes([7, 255], 8)) == [7, 255]


# ---- FrameFormat -----------------------------------------------------------------------------------------------------------------------
def test_frame_format_depth_validation():
    assert FrameFormat().depth == 8 and FrameFormat("yuv444p", "bt601", "full", "trunc", 12).depth == 12
    for depth in (8, 10, 12, 16):
        assert FrameFormat("yuv420p", depth=depth).depth == depth
    for depth in (0, 9, 11, 14, 17, 32, "10", 10.5, None, True):
        with pytest.raises(ValueError, match="depth"):
            FrameFormat("yuv420p", depth=depth)
    with pytest.raises(ValueError, match="rgb24"):
        FrameFormat("rgb24", depth=10)
    with pytest.raises(ValueError, match="matrix"):
        FrameFormat("yuv420p", matrix="bt2020", depth=10)
    assert FrameFormat("yuv420p", depth=10) != FrameFormat("yuv420p") and FrameFormat("yuv420p", depth=8) == FrameFormat("yuv420p")
    assert FrameFormat("yuv444p", depth=16).rounding_used == "nearest"


def test_from_name_and_name_round_trip():
    for name in ("yuv420p", "yuv444p", "rgb24"):
        f = FrameFormat.from_name(name)
        assert (f.layout, f.depth, f.name) == (name, 8, name)
    for layout in ("yuv420p", "yuv444p"):
        for depth in (10, 12, 16):
            for suffix in ("le", ""):
                f = FrameFormat.from_name(f"{layout}{depth}{suffix}", matrix="bt601", range="full", rounding="trunc")
                assert f == FrameFormat(layout, "bt601", "full", "trunc", depth)
                assert f.name == f"{layout}{depth}le" and FrameFormat.from_name(f.name, "bt601", "full", "trunc") == f
    for bad in ("yuv420p10be", "yuv422p10le", "yuv420p9le", "yuv420p8", "rgb48le", "yuv420p10lele", "", "YUV420P10LE"):
        with pytest.raises(ValueError, match="unknown format name"):
            FrameFormat.from_name(bad)


# ---- frame_bytes, planes ---------------------------------------------------------------------------------------------------------------
def test_frame_bytes_and_planes_of_deep_formats():
    H, W = 6, 10
    for depth in (10, 12, 16):
        f444, f420 = FrameFormat("yuv444p", depth=depth), FrameFormat("yuv420p", depth=depth)
        assert fo.frame_bytes(H, W, f444) == 2 * 3 * H * W == 2 * fo.frame_bytes(H, W, FrameFormat("yuv444p"))
        assert fo.frame_bytes(H, W, f420) == 2 * (H * W * 3 // 2) == 2 * fo.frame_bytes(H, W, FrameFormat("yuv420p"))
    with pytest.raises(ValueError, match="even"):
        fo.frame_bytes(5, 10, FrameFormat("yuv420p", depth=10))
    fmt = FrameFormat("yuv420p", depth=10)
    codes = np.arange(H * W * 3 // 2, dtype=np.int64) + 300          # (above 255: both bytes of a word matter)
    buf = ref.to_bytes(codes, 10)
    assert buf.dtype == np.uint8 and buf.shape == (fo.frame_bytes(H, W, fmt),)
    for frame in (buf, torch.from_numpy(buf.copy())):
        y, u, v = fo.planes(frame, H, W, fmt)
        as_np = [np.asarray(p) if isinstance(p, np.ndarray) else p.numpy() for p in (y, u, v)]
        assert all(p.dtype == np.uint16 for p in as_np)
        assert [p.shape for p in as_np] == [(H, W), (H // 2, W // 2), (H // 2, W // 2)]
        assert np.array_equal(as_np[0].reshape(-1), codes[:H * W])          # offsets: Y at word 0, U at H W, V at H W + H W / 4
        assert np.array_equal(as_np[1].reshape(-1), codes[H * W:H * W + H * W // 4])
        assert np.array_equal(as_np[2].reshape(-1), codes[H * W + H * W // 4:])
    y, u, v = fo.planes(buf, H, W, fmt)
    assert y.dtype.byteorder in ("<", "=") and np.shares_memory(y, buf) and np.shares_memory(v, buf)          # views, not copies
    ty = fo.planes(torch.from_numpy(buf), H, W, fmt)[0]
    assert ty.dtype == torch.uint16
    y4, u4, v4 = fo.planes(ref.to_bytes(np.arange(3 * H * W) + 300, 12), H, W, FrameFormat("yuv444p", depth=12))
    assert y4.shape == u4.shape == v4.shape == (H, W) and u4[0, 0] == 300 + H * W and v4[0, 0] == 300 + 2 * H * W
    with pytest.raises(ValueError, match="bytes"):
        fo.planes(buf[:-2], H, W, fmt)
    # 8-bit frames as before
    y8, u8, v8 = fo.planes(np.zeros(H * W * 3 // 2, np.uint8), H, W, FrameFormat("yuv420p"))
    assert y8.dtype == np.uint8 and u8.shape == (H // 2, W // 2)


# ---- Y4M -------------------------------------------------------------------------------------------------------------------------------
def test_y4m_headers():
    assert fo.y4m_header(8, 4) == b"YUV4MPEG2 W8 H4 F30:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"          # 8-bit: byte for byte as before
    assert fo.y4m_header(8, 4, (25, 2), FrameFormat("yuv444p", range="full")) == b"YUV4MPEG2 W8 H4 F25:2 Ip A1:1 C444 XCOLORRANGE=FULL\n"
    assert fo.y4m_header(8, 4, fmt=FrameFormat("yuv420p", depth=10)) == b"YUV4MPEG2 W8 H4 F30:1 Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n"
    assert fo.y4m_header(8, 4, 24, FrameFormat("yuv444p", range="full", depth=12)) == b"YUV4MPEG2 W8 H4 F24:1 Ip A1:1 C444p12 XCOLORRANGE=FULL\n"
    assert b" C420p16 " in fo.y4m_header(8, 4, fmt=FrameFormat("yuv420p", depth=16)) and b" C444p10 " in fo.y4m_header(8, 4, fmt=FrameFormat("yuv444p", depth=10))


def test_read_y4m_on_a_hand_made_10_bit_file(tmp_path):
    W, H = 4, 2
    f0 = ref.to_bytes([64, 940, 512, 1023, 0, 1, 2, 3, 100, 900, 512, 513], 10)
    f1 = ref.to_bytes(np.arange(12) * 80, 10)
    (tmp_path / "a.y4m").write_bytes(b"YUV4MPEG2 W4 H2 F24:1 Ip A1:1 C420p10 XCOLORRANGE=FULL\n" + b"FRAME\n" + f0.tobytes() + b"FRAME\n" + f1.tobytes())
    hdr, frames = fo.read_y4m(tmp_path / "a.y4m")
    assert (hdr["W"], hdr["H"], hdr["layout"], hdr["depth"], hdr["range"], hdr["frame_bytes"], hdr["chroma"]) == (W, H, "yuv420p", 10, "full", 24, "420p10")
    assert frames.dtype == np.uint8 and frames.shape == (2, 24) and np.array_equal(frames[0], f0) and np.array_equal(frames[1], f1)
    assert frames.ctypes.data % 2 == 0          # a fresh array: every frame of an even length starts at an even address
    y, u, v = fo.planes(frames[0], H, W, FrameFormat("yuv420p", depth=10))
    assert y.tolist() == [[64, 940, 512, 1023], [0, 1, 2, 3]] and u.tolist() == [[100, 900]] and v.tolist() == [[512, 513]]
    hdr2, got = fi.open_video(tmp_path / "a.y4m", fmt=FrameFormat("yuv444p", "bt601", "limited", depth=16))
    assert hdr2["fmt"] == FrameFormat("yuv420p", "bt601", "full", depth=10) and hdr2["depth"] == 10 and hdr2["frames"] == 2          # the file's depth wins
    assert np.array_equal(got, frames)
    # the 8-bit tags say depth 8; a writer's deep file comes back; 4:2:2 is still refused
    (tmp_path / "b.y4m").write_bytes(b"YUV4MPEG2 W4 H2 F24:1 C420mpeg2\nFRAME\n" + bytes(12))
    assert fo.read_y4m(tmp_path / "b.y4m")[0]["depth"] == 8 and fi.open_video(tmp_path / "b.y4m")[0]["fmt"] == FrameFormat("yuv420p")
    fmt = FrameFormat("yuv444p", depth=12)
    with fo.Y4MWriter(tmp_path / "c.y4m", W, H, (30, 1), fmt) as sink:
        assert sink.frame_bytes == 48
        sink.write(ref.to_bytes(np.arange(24) * 170, 12))
        with pytest.raises(ValueError, match="48 bytes"):
            sink.write(np.zeros(24, np.uint8))
    hdr3, back = fi.open_video(tmp_path / "c.y4m")
    assert hdr3["fmt"] == fmt and hdr3["chroma"] == "444p12" and np.array_equal(ref.from_bytes(back[0], 12), np.arange(24) * 170)
    for tag in ("C422", "C422p10", "C420p9", "C444p14", "Cmono"):
        (tmp_path / "bad.y4m").write_bytes(f"YUV4MPEG2 W4 H4 F30:1 {tag}\nFRAME\n".encode() + bytes(64))
        with pytest.raises(ValueError, match="4:2:0 / 4:4:4"):
            fi.open_video(tmp_path / "bad.y4m")
    (tmp_path / "cut.y4m").write_bytes(b"YUV4MPEG2 W4 H2 F30:1 C420p10\nFRAME\n" + bytes(23))
    with pytest.raises(ValueError, match="truncated"):
        fi.open_video(tmp_path / "cut.y4m")


def test_raw_deep_files(tmp_path):
    W, H, T = 10, 6, 3
    fmt = FrameFormat("yuv420p", depth=10)
    nb = fo.frame_bytes(H, W, fmt)
    frames = np.stack([ref.to_bytes(ref.random_codes(H, W, "yuv420p", 10, k), 10) for k in range(T)])
    (tmp_path / "v.yuv").write_bytes(frames.tobytes())
    hdr, got = fi.open_video(tmp_path / "v.yuv", W, H, fmt=fmt)
    assert hdr["fmt"] == fmt and (hdr["depth"], hdr["frames"], hdr["frame_bytes"]) == (10, T, nb) and np.array_equal(got, frames)
    assert fi.open_video(tmp_path / "v.yuv", W, H)[0]["frames"] == 2 * T          # the same bytes read as 8-bit: the depth comes from fmt
    (tmp_path / "partial.yuv").write_bytes(frames.tobytes() + bytes(nb // 2))          # a whole number of 8-bit frames, not of deep ones
    assert fi.open_video(tmp_path / "partial.yuv", W, H)[0]["frames"] == 2 * T + 1
    with pytest.raises(ValueError, match="not a whole number of yuv420p10le frames"):
        fi.open_video(tmp_path / "partial.yuv", W, H, fmt=fmt)
    sink, used = fo.open_sink(tmp_path / "w.yuv", W, H, fmt=fmt)
    assert used == fmt and isinstance(sink, fo.RawWriter)
    with sink:
        for fr in frames:
            sink.write(fr)
    assert (tmp_path / "w.yuv").read_bytes() == frames.tobytes()
    sink, used = fo.open_sink(tmp_path / "w.y4m", W, H, fmt=fmt)
    sink.close()
    assert used == fmt and (tmp_path / "w.y4m").read_bytes() == fo.y4m_header(W, H, (30, 1), fmt)


# ---- before a GPU is needed ------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused_before_a_gpu_is_needed():
    fmt = FrameFormat("yuv420p", depth=10)
    with pytest.raises(_lib.GsvcError, match="CPU tensors are not supported"):
        fo.frames_to_u8(torch.zeros(1, 3, 4, 4), fmt)
    with pytest.raises(_lib.GsvcError, match="CPU tensors are not supported"):
        fi.frames_from_u8(torch.zeros(2, 48, dtype=torch.uint8), 4, 4, fmt)
    with pytest.raises(_lib.GsvcError, match="CPU tensors are not supported"):
        fo.delivered_images(torch.zeros(1, 3, 4, 4), fmt)
    from gsvc_amd.report import evaluate
    with pytest.raises(ValueError, match="give one"):
        evaluate(None, None, None, None, eight_bit=True, delivered=fmt)


# ---- the host-side checks of the C entry points (nothing is launched) ----------------------------------------------------------------
RGB, P444, P420 = 0, 1, 2


def _lib_built():
    import __graft_entry__ as g
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


def test_c_frames_bytes():
    L = _lib_built()
    for layout in (RGB, P444, P420):
        assert L.gsvc_frames_bytes(6, 10, layout, 8) == L.gsvc_frames_u8_bytes(6, 10, layout) > 0
    for depth in (9, 10, 12, 16):
        assert L.gsvc_frames_bytes(6, 10, P444, depth) == 360 and L.gsvc_frames_bytes(6, 10, P420, depth) == 180
        assert L.gsvc_frames_bytes(6, 10, RGB, depth) < 0
    for depth in (-1, 0, 7, 17, 32):
        assert L.gsvc_frames_bytes(6, 10, P444, depth) < 0
    assert L.gsvc_frames_bytes(5, 10, P420, 10) < 0 and L.gsvc_frames_bytes(0, 10, P444, 10) < 0 and L.gsvc_frames_bytes(6, 40000, P444, 10) < 0
    assert L.gsvc_frames_bytes(6, 10, 3, 10) < 0
    assert L.gsvc_frames_bytes(2160, 3840, P420, 10) == 2160 * 3840 * 3


REFUSALS = ((dict(base=0x2001), b"not 2-byte aligned"), (dict(stride=97), b"not a multiple of 2"), (dict(depth=8), b"depth must be 9 .. 16"),
            (dict(depth=17), b"depth must be 9 .. 16"), (dict(layout=RGB), b"rgb24"), (dict(n=0), b"n must be 1 .. 16"),
            (dict(n=17), b"n must be 1 .. 16"), (dict(layout=P420, H=3), b"even H and W"), (dict(layout=P420, W=5), b"even H and W"),
            (dict(layout=3), b"unknown layout"), (dict(matrix=2), b"unknown matrix"), (dict(rng=2), b"unknown range"), (dict(mode=2), b"unknown"),
            (dict(H=0), b"image size"), (dict(W=40000), b"image size"), (dict(stride=94), b"shorter than a frame"),
            (dict(layout=P420, stride=46), b"shorter than a frame"), (dict(base=None), b"NULL pointer"), (dict(images=None), b"NULL pointer"))


def test_c_entries_refuse_on_the_host_side():
    """Every refusal returns -1 with its message and launches nothing: no GPU is present here, and the pointers are made up."""
    L = _lib_built()
    one = (C.c_void_p * 1)(0x1000)

    def to_u16(base=0x2000, stride=96, n=1, H=4, W=4, layout=P444, matrix=0, rng=0, mode=1, depth=10, images=one):
        return L.gsvc_frames_to_u16(images, n, H, W, layout, matrix, rng, mode, depth, base, stride, None)

    def from_u16(base=0x2000, stride=96, n=1, H=4, W=4, layout=P444, matrix=0, rng=0, mode=1, depth=10, images=one):
        return L.gsvc_frames_from_u16(base, stride, n, H, W, layout, matrix, rng, mode, depth, images, None)

    for call in (to_u16, from_u16):
        for kwargs, message in REFUSALS + ((dict(images=(C.c_void_p * 1)(0x1002)), b"not 4-byte aligned"), (dict(images=(C.c_void_p * 1)(0)), b"NULL image pointer")):
            assert call(**kwargs) == -1, (call.__name__, kwargs)
            assert message in L.gsvc_last_error(), (call.__name__, kwargs, L.gsvc_last_error())
            assert (b"frames_to_u16" if call is to_u16 else b"frames_from_u16") in L.gsvc_last_error()


# ---- the fit tool's format arguments ----------------------------------------------------------------------------------------------------
def test_fit_tool_parses_deep_format_names():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fit_synthetic
    assert fit_synthetic._frame_format("yuv420p10le") == FrameFormat("yuv420p", depth=10)
    assert fit_synthetic._frame_format("yuv444p12,bt601,full") == FrameFormat("yuv444p", "bt601", "full", depth=12)
    assert fit_synthetic._frame_format("yuv420p,bt601") == FrameFormat("yuv420p", "bt601") and fit_synthetic._frame_format("rgb24") == FrameFormat("rgb24")
    with pytest.raises(ValueError, match="unknown format name"):
        fit_synthetic._frame_format("yuv422p10le")
    with pytest.raises(SystemExit):
        fit_synthetic._frame_format("yuv420p,bt709,full,nearest")
