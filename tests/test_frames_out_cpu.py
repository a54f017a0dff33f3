"""CPU tests of the decoder's 8-bit output stage: the host parts of gsvc_amd/frames_out.py (sizes, plane views, validation, the
Y4M / raw / PNG sinks, the writer thread) and the float64 reference of the conversion (tests/_frames_ref.py) on values one can do
by hand.  The kernel itself is held to that reference in tests/test_frames_out_gpu.py."""
import os
import threading

import numpy as np
import pytest
import torch

from gsvc_amd import _lib, frames_out as fo
from gsvc_amd.frames_out import FrameFormat
from tests import _frames_ref as ref

LAYOUTS = ("rgb24", "yuv444p", "yuv420p")


# ---- sizes, views, validation ------------------------------------------------------------------------------------------
def test_frame_bytes_1080p():
    assert fo.frame_bytes(1080, 1920, FrameFormat("rgb24")) == 6_220_800
    assert fo.frame_bytes(1080, 1920, FrameFormat("yuv444p")) == 6_220_800
    assert fo.frame_bytes(1080, 1920, FrameFormat("yuv420p")) == 3_110_400
    assert fo.frame_bytes(33, 47, FrameFormat("rgb24")) == 33 * 47 * 3
    assert fo.frame_bytes(2, 2) == 6          # the default format is yuv420p


def test_format_defaults():
    f = FrameFormat()
    assert (f.layout, f.matrix, f.range, f.rounding) == ("yuv420p", "bt709", "limited", None)
    assert f.rounding_used == "nearest"
    assert FrameFormat("rgb24").rounding_used == "trunc"
    assert FrameFormat("rgb24", rounding="nearest").rounding_used == "nearest"
    assert FrameFormat("yuv444p", rounding="trunc").rounding_used == "trunc"


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_planes_are_views_in_frame_order(kind):
    H, W = 4, 6
    for layout in LAYOUTS:
        fmt = FrameFormat(layout)
        n = fo.frame_bytes(H, W, fmt)
        buf = np.arange(n, dtype=np.uint8) if kind == "numpy" else torch.arange(n, dtype=torch.uint8)
        p = fo.planes(buf, H, W, fmt)
        if layout == "rgb24":
            assert len(p) == 1 and tuple(p[0].shape) == (H, W, 3)
            assert int(p[0][1, 2, 1]) == (1 * W + 2) * 3 + 1
        else:
            ch, cw = (H // 2, W // 2) if layout == "yuv420p" else (H, W)
            assert [tuple(x.shape) for x in p] == [(H, W), (ch, cw), (ch, cw)]
            assert int(p[0][1, 2]) == W + 2 and int(p[1][0, 0]) == H * W and int(p[2][0, 0]) == H * W + ch * cw
        p[0][...] = 7          # a view: writing it writes the frame
        assert int(buf[0]) == 7


def test_validation_errors():
    with pytest.raises(ValueError, match="even"):
        fo.frame_bytes(3, 4, FrameFormat("yuv420p"))
    with pytest.raises(ValueError, match="even"):
        fo.frame_bytes(4, 5, FrameFormat("yuv420p"))
    with pytest.raises(ValueError, match="positive"):
        fo.frame_bytes(0, 4, FrameFormat("rgb24"))
    for kw in ({"layout": "nv12"}, {"matrix": "bt2020"}, {"range": "tv"}, {"rounding": "floor"}):
        with pytest.raises(ValueError, match="unknown"):
            FrameFormat(**kw)
    with pytest.raises(ValueError, match="bytes"):
        fo.planes(np.zeros(10, np.uint8), 2, 2, FrameFormat("rgb24"))
    with pytest.raises(_lib.GsvcError, match="CPU tensors"):
        fo.frames_to_u8([torch.zeros(3, 4, 4)], FrameFormat("rgb24"))
    with pytest.raises(ValueError, match="Y4M"):
        fo.Y4MWriter(os.devnull, 4, 4, fmt=FrameFormat("rgb24"))


def test_enums_match_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gsvc_hip.h")).read()
    for table, names in ((fo.LAYOUTS, {"rgb24": "RGB24", "yuv444p": "YUV444P", "yuv420p": "YUV420P"}),
                         (fo.MATRICES, {"bt709": "BT709", "bt601": "BT601"}), (fo.RANGES, {"limited": "LIMITED", "full": "FULL"}),
                         (fo.ROUNDINGS, {"trunc": "TRUNC", "nearest": "NEAREST"})):
        for key, c_name in names.items():
            assert f"GSVC_FRAMES_{c_name} = {table[key]}" in text, c_name
    assert f"#define GSVC_FRAMES_MAX_BATCH {fo.MAX_BATCH}" in text


def test_library_validates_on_the_host():
    """gsvc_frames_u8_bytes and the argument checks of gsvc_frames_to_u8 run without a GPU (nothing is launched)."""
    import ctypes as C
    L = _lib.lib()
    assert L.gsvc_frames_u8_bytes(1080, 1920, 0) == 6_220_800 and L.gsvc_frames_u8_bytes(1080, 1920, 2) == 3_110_400
    assert L.gsvc_frames_u8_bytes(3, 4, 2) < 0 and L.gsvc_frames_u8_bytes(4, 4, 9) < 0 and L.gsvc_frames_u8_bytes(0, 4, 0) < 0
    ptrs = (C.c_void_p * 1)(64)
    for args, msg in (((None, 1, 4, 4, 0, 0, 0, 0, 64, 48, None), b"NULL"), ((ptrs, 0, 4, 4, 0, 0, 0, 0, 64, 48, None), b"n must be"),
                      ((ptrs, 17, 4, 4, 0, 0, 0, 0, 64, 48, None), b"n must be"), ((ptrs, 1, 3, 4, 2, 0, 0, 0, 64, 48, None), b"even"),
                      ((ptrs, 1, 4, 4, 3, 0, 0, 0, 64, 48, None), b"unknown layout"), ((ptrs, 1, 4, 4, 1, 2, 0, 0, 64, 48, None), b"unknown matrix"),
                      ((ptrs, 1, 4, 4, 1, 0, 2, 0, 64, 48, None), b"unknown range"), ((ptrs, 1, 4, 4, 1, 0, 0, 2, 64, 48, None), b"unknown rounding"),
                      ((ptrs, 1, 4, 4, 0, 0, 0, 0, 64, 47, None), b"out_stride"), ((ptrs, 1, 4, 4, 0, 0, 0, 0, None, 48, None), b"NULL")):
        assert L.gsvc_frames_to_u8(*args) == -1, args
        assert msg in L.gsvc_last_error(), (args, L.gsvc_last_error())


# ---- the reference on values one can do by hand --------------------------------------------------------------------------
def _flat(rgb, H=2, W=2):
    return np.broadcast_to(np.asarray(rgb, np.float64)[:, None, None], (3, H, W)).copy()


@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
@pytest.mark.parametrize("layout", ["yuv444p", "yuv420p"])
def test_reference_grey_white_black(layout, matrix):
    for rng, white, black in (("limited", 235, 16), ("full", 255, 0)):
        for rounding in ("nearest", "trunc"):
            g = fo.planes(ref.convert(_flat([0.5] * 3), layout, matrix, rng, rounding), 2, 2, FrameFormat(layout))
            # (B - Y is zero up to one float64 rounding of Y: exactly 128 under nearest; truncation may land one below)
            for p in (g[1], g[2]):
                assert (p == 128).all() if rounding == "nearest" else ((p >= 127) & (p <= 128)).all()
            w = fo.planes(ref.convert(_flat([1.0] * 3), layout, matrix, rng, rounding), 2, 2, FrameFormat(layout))
            b = fo.planes(ref.convert(_flat([0.0] * 3), layout, matrix, rng, rounding), 2, 2, FrameFormat(layout))
            # (white's luma is Kr + Kg + Kb = 1 up to one float64 rounding: exact under nearest, one below under truncation is allowed)
            assert (w[0] == white).all() if rounding == "nearest" else ((w[0] >= white - 1) & (w[0] <= white)).all()
            assert (b[0] == black).all()
            for p in (w[1], w[2], b[1], b[2]):
                assert (np.abs(p.astype(int) - 128) <= (1 if rounding == "trunc" else 0)).all()


@pytest.mark.parametrize("matrix,Kr,Kb", [("bt709", 0.2126, 0.0722), ("bt601", 0.299, 0.114)])
def test_reference_primaries(matrix, Kr, Kb):
    Kg = 1.0 - Kr - Kb
    for rgb, k in (((1, 0, 0), Kr), ((0, 1, 0), Kg), ((0, 0, 1), Kb)):
        for rng, (yo, ys, cs) in (("limited", (16, 219, 224)), ("full", (0, 255, 255))):
            y, u, v = (int(p[0, 0]) for p in fo.planes(ref.convert(_flat(rgb), "yuv444p", matrix, rng, "nearest"), 2, 2, FrameFormat("yuv444p")))
            R, _, B = rgb
            assert y == int(np.floor(yo + ys * k + 0.5))
            assert u == min(255, int(np.floor(128 + cs * (B - k) / (2 * (1 - Kb)) + 0.5)))
            assert v == min(255, int(np.floor(128 + cs * (R - k) / (2 * (1 - Kr)) + 0.5)))
    # the numbers everybody knows: BT.601 limited red = (81, 90, 240), blue = (41, 240, 110); BT.709 limited red = (63, 102, 240)
    def px(rgb, m):
        return tuple(int(p[0, 0]) for p in fo.planes(ref.convert(_flat(rgb), "yuv444p", m, "limited", "nearest"), 2, 2, FrameFormat("yuv444p")))
    if matrix == "bt601":
        assert px((1, 0, 0), matrix) == (81, 90, 240) and px((0, 0, 1), matrix) == (41, 240, 110)
    else:
        assert px((1, 0, 0), matrix) == (63, 102, 240)


def test_reference_limited_range_stays_in_range_and_clamps():
    rng = np.random.default_rng(5)
    img = rng.uniform(0.0, 1.0, (3, 16, 24))
    img[:, :4, :4] = rng.integers(0, 2, (3, 4, 4))          # saturated corners: the extremes of Cb / Cr
    for layout in ("yuv444p", "yuv420p"):
        for matrix in ("bt709", "bt601"):
            for rounding in ("nearest", "trunc"):
                y, u, v = fo.planes(ref.convert(img, layout, matrix, "limited", rounding), 16, 24, FrameFormat(layout))
                assert y.min() >= 16 and y.max() <= 235
                assert min(u.min(), v.min()) >= 16 and max(u.max(), v.max()) <= 240
    bad = np.array([np.nan, -np.inf, np.inf, -3.0, 7.0, 0.25])
    img = np.broadcast_to(bad[None, None, :], (3, 2, 6)).copy()
    got = fo.planes(ref.convert(img, "rgb24", rounding="trunc"), 2, 6, FrameFormat("rgb24"))[0]
    assert got[0, :, 0].tolist() == [0, 0, 255, 0, 255, 63]
    y = fo.planes(ref.convert(img, "yuv444p"), 2, 6, FrameFormat("yuv444p"))[0]
    assert y[0].tolist() == [16, 16, 235, 16, 235, 71]


def test_chroma_is_averaged_before_quantisation():
    img = np.zeros((3, 2, 2))
    img[:, 0, 0] = (1.0, 0.0, 0.0)          # one red pixel in a black block
    _, u, v = fo.planes(ref.convert(img, "yuv420p", "bt601", "limited", "nearest"), 2, 2, FrameFormat("yuv420p"))
    cb, cr = -0.299 / (2 * (1 - 0.114)), 0.5
    assert int(u[0, 0]) == int(np.floor(128 + 224 * cb / 4 + 0.5)) and int(v[0, 0]) == int(np.floor(128 + 224 * cr / 4 + 0.5)) == 156


@pytest.mark.parametrize("rounding", ["trunc", "nearest"])
def test_k_over_255_survives_rgb24(rounding):
    """k / 255 in float32, times 255 in float32 (the kernel's one product), gives k back under both roundings, for all 256 k."""
    k = np.arange(256)
    x32 = (k.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    v32 = (np.float32(255.0) * x32).astype(np.float32)
    got = np.floor(v32 + (np.float32(0.5) if rounding == "nearest" else np.float32(0.0))).astype(np.uint8)
    assert (got == k).all()
    t = (torch.from_numpy(x32).clamp(0, 1).mul(255) + (0.5 if rounding == "nearest" else 0.0)).to(torch.uint8).numpy()
    assert (t == k).all()
    img = np.broadcast_to(x32[None, None, :], (3, 1, 256))
    assert (fo.planes(ref.convert(img, "rgb24", rounding=rounding), 1, 256, FrameFormat("rgb24"))[0][0, :, 1] == k).all()


def test_check_bytes_catches_a_wrong_matrix_and_accepts_neighbours_in_the_band():
    rng = np.random.default_rng(9)
    img = rng.uniform(-0.1, 1.1, (3, 8, 8))
    v = ref.values(img, "yuv420p", "bt709", "limited")
    assert ref.check_bytes(ref.quantise(v, "nearest"), v, "nearest")[0] == 0
    assert ref.check_bytes(ref.quantise(v, "trunc"), v, "trunc")[0] == 0
    assert ref.check_bytes(ref.convert(img, "yuv420p", "bt601", "limited"), v, "nearest")[0] > 0
    assert ref.check_bytes(ref.convert(img, "yuv420p", "bt709", "full"), v, "nearest")[0] > 0
    assert ref.check_bytes(ref.quantise(v, "trunc"), v, "nearest")[0] > 0
    vv = np.array([10.5 - 1e-4, 10.5 + 1e-4, 11.0 - 1e-4])
    assert ref.check_bytes(np.array([11, 10, 11]), vv[:3], "nearest")[0] == 0          # inside the band either neighbour passes
    assert ref.check_bytes(np.array([10, 10, 11]), vv, "trunc")[0] == 0
    assert ref.check_bytes(np.array([12, 10, 11]), vv, "nearest")[0] == 1


def test_float32_arithmetic_is_far_inside_the_tolerances():
    """Where the GPU test's bounds come from: the formulas evaluated step by step in float32 stay within 3.3e-5 of float64 (the
    bound is delta = 2^-11 = 4.9e-4), break the per-byte condition nowhere, and differ from the exactly rounded value in well
    under 2e-3 of the bytes of a noise or ramp image — so the GPU test's limits leave honest single precision a wide margin."""
    for H, W in ((34, 50), (270, 480)):
        for layout in LAYOUTS:
            for matrix in ("bt709", "bt601"):
                for rng in ("limited", "full"):
                    for kind in ref.KINDS:
                        img = ref.make_image(kind, H, W)
                        v, v32 = ref.values(img, layout, matrix, rng), ref.values32(img, layout, matrix, rng)
                        assert np.abs(v32 - v).max() <= 3.3e-5
                        for rounding in ("trunc", "nearest"):
                            b = ref.quantise32(v32, rounding)
                            assert ref.check_bytes(b, v, rounding)[0] == 0
                            if kind in ("noise", "ramp"):
                                assert (b != ref.quantise(v, rounding)).mean() <= 1e-3, (H, W, layout, matrix, rng, rounding, kind)


# ---- sinks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,rng,tag", [("yuv420p", "limited", b"C420jpeg XCOLORRANGE=LIMITED"), ("yuv444p", "full", b"C444 XCOLORRANGE=FULL")])
def test_y4m_round_trip(tmp_path, layout, rng, tag):
    H, W, T = 6, 8, 5
    fmt = FrameFormat(layout, range=rng)
    n = fo.frame_bytes(H, W, fmt)
    frames = np.random.default_rng(1).integers(0, 256, (T, n), dtype=np.uint8)
    path = tmp_path / "a.y4m"
    with fo.Y4MWriter(path, W, H, fps=(25, 1), fmt=fmt) as w:
        for k in range(T):
            w.write(frames[k] if k % 2 else torch.from_numpy(frames[k]))
        with pytest.raises(ValueError, match="bytes"):
            w.write(frames[0][:-1])
    header = b"YUV4MPEG2 W8 H6 F25:1 Ip A1:1 " + tag + b"\n"
    data = path.read_bytes()
    assert data.startswith(header) and data[len(header):len(header) + 6] == b"FRAME\n"
    assert len(data) == len(header) + T * (6 + n) == w.bytes and w.frames == T
    hdr, back = fo.read_y4m(path)
    assert (hdr["W"], hdr["H"], hdr["fps"], hdr["interlace"], hdr["aspect"], hdr["layout"], hdr["range"], hdr["frame_bytes"]) == \
        (W, H, (25, 1), "p", "1:1", layout, rng, n)
    assert back.dtype == np.uint8 and back.shape == (T, n) and (back == frames).all()


def test_y4m_default_header_is_exact():
    assert fo.y4m_header(1920, 1080) == b"YUV4MPEG2 W1920 H1080 F30:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    assert fo.y4m_header(16, 8, (30000, 1001), FrameFormat("yuv444p", range="full")) == b"YUV4MPEG2 W16 H8 F30000:1001 Ip A1:1 C444 XCOLORRANGE=FULL\n"


def test_raw_writer(tmp_path):
    frames = np.random.default_rng(2).integers(0, 256, (3, 4 * 6 * 3), dtype=np.uint8)
    with fo.RawWriter(tmp_path / "a.rgb") as w:
        for f in frames:
            w.write(f)
    assert (tmp_path / "a.rgb").read_bytes() == frames.tobytes() and w.frames == 3 and w.bytes == frames.size


def test_png_writer_round_trip(tmp_path):
    from PIL import Image
    H, W = 5, 7
    frames = np.random.default_rng(3).integers(0, 256, (3, H * W * 3), dtype=np.uint8)
    with fo.PNGWriter(tmp_path / "png", W, H) as w:
        w.write(frames[0])                                   # flat
        w.write(torch.from_numpy(frames[1]))                  # flat tensor
        w.write(frames[2].reshape(H, W, 3))                   # [H, W, 3]
    assert sorted(os.listdir(tmp_path / "png")) == ["d00000.png", "d00001.png", "d00002.png"]
    for k in range(3):
        img = Image.open(tmp_path / "png" / f"d{k:05d}.png")
        assert img.mode == "RGB" and img.size == (W, H)
        assert (np.asarray(img).reshape(-1) == frames[k]).all()
    with pytest.raises(ValueError, match="flat frame"):
        fo.PNGWriter(tmp_path / "png2").write(frames[0])


def test_open_sink_by_extension(tmp_path):
    s, f = fo.open_sink(tmp_path / "a.y4m", 8, 6)
    assert isinstance(s, fo.Y4MWriter) and f.layout == "yuv420p"
    s.close()
    s, f = fo.open_sink(tmp_path / "a.yuv", 8, 6)
    assert isinstance(s, fo.RawWriter) and f.layout == "yuv420p"
    s.close()
    s, f = fo.open_sink(tmp_path / "a.rgb", 8, 6)
    assert isinstance(s, fo.RawWriter) and f.layout == "rgb24"
    s.close()
    s, f = fo.open_sink(tmp_path / "frames", 8, 6)
    assert isinstance(s, fo.PNGWriter) and f.layout == "rgb24" and os.path.isdir(tmp_path / "frames")


# ---- the writer thread ------------------------------------------------------------------------------------------------------
def test_write_frames_copies_and_counts(tmp_path):
    n = fo.frame_bytes(4, 4)
    shared = np.zeros(n, np.uint8)

    def produce():          # one buffer reused for every frame, as render_frames_u8's pinned ring is
        for k in range(40):
            shared[:] = k
            yield shared

    res = fo.write_frames(produce(), fo.Y4MWriter(tmp_path / "a.y4m", 4, 4), queue_frames=3)
    hdr, back = fo.read_y4m(tmp_path / "a.y4m")
    assert res["frames"] == 40 and res["bytes"] == os.path.getsize(tmp_path / "a.y4m") and res["seconds"] > 0 and res["fps"] > 0
    assert (back == np.arange(40, dtype=np.uint8)[:, None]).all()


def test_write_frames_propagates_the_sinks_exception():
    class Failing:
        def __init__(self):
            self.seen, self.closed, self.thread = 0, False, None

        def write(self, frame):
            self.thread = threading.current_thread()
            self.seen += 1
            if self.seen == 3:
                raise OSError("disk full")

        def close(self):
            self.closed = True

    sink = Failing()
    done = []

    def run():
        try:
            fo.write_frames((np.full(8, k, np.uint8) for k in range(1000)), sink, queue_frames=2)
        except OSError as e:
            done.append(e)

    t = threading.Thread(target=run, daemon=True)
    t.start()
    t.join(30)
    assert not t.is_alive(), "write_frames hangs after its sink failed"
    assert len(done) == 1 and "disk full" in str(done[0])
    assert sink.closed and sink.seen == 3 and sink.thread is not threading.main_thread()
    assert not [th for th in threading.enumerate() if th.name == "gsvc-frame-writer"]
