"""CPU tests of the encoder's 8-bit input stage: the float64 reference of tests/_frames_in_ref.py on values that can be checked by
hand, the margin of the GPU tests' tolerance (honest float32 against float64), the file side of gsvc_amd/frames_in.py (``open_video``,
``VideoFileCube`` argument errors) and the host-side checks of gsvc_frames_from_u8.  No GPU is used."""
import ctypes as C

import numpy as np
import pytest
import torch

from gsvc_amd import _lib
from gsvc_amd import frames_in as fi
from gsvc_amd import frames_out as fo
from gsvc_amd.frames_out import FrameFormat
from tests import _frames_in_ref as ref
from tests import _frames_ref as ref_out

COMBOS = [(m, r) for m in ("bt709", "bt601") for r in ("limited", "full")]


# ---- the reference on hand-checkable values ---------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
def test_limited_range_black_and_white(matrix):
    assert np.array_equal(ref.rgb_of_codes(16, 128, 128, matrix, "limited"), [0.0, 0.0, 0.0])
    assert np.array_equal(ref.rgb_of_codes(235, 128, 128, matrix, "limited"), [1.0, 1.0, 1.0])
    assert np.array_equal(ref.rgb_of_codes(0, 128, 128, matrix, "limited"), [0.0, 0.0, 0.0])          # below black: clamped
    assert np.array_equal(ref.rgb_of_codes(255, 128, 128, matrix, "limited"), [1.0, 1.0, 1.0])        # above white: clamped
    grey = ref.rgb_of_codes(126, 128, 128, matrix, "limited")
    assert np.allclose(grey, 110.0 / 219.0, rtol=0, atol=1e-15)


@pytest.mark.parametrize("matrix", ["bt709", "bt601"])
def test_full_range_primaries(matrix):
    """The exact Y, Cb, Cr of a primary, scaled to full-range codes WITHOUT rounding, come back as the primary."""
    Kr, Kb = ref.MATRIX[matrix]
    Kg = 1.0 - Kr - Kb
    for rgb in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1), (0, 0, 0)):
        R, G, B = rgb
        Y = Kr * R + Kg * G + Kb * B
        cb, cr = (B - Y) / (2 * (1 - Kb)), (R - Y) / (2 * (1 - Kr))
        got = ref.rgb_of_codes(255 * Y, 128 + 255 * cb, 128 + 255 * cr, matrix, "full")
        assert np.allclose(got, rgb, rtol=0, atol=1e-12), (rgb, got)
    # and a rounded code triple by hand: red in BT.601 full range is (76, 85, 255) -> R = 76/255 + 1.402 * 127/255
    got = ref.rgb_of_codes(76, 85, 255, "bt601", "full")
    assert abs(got[0] - min(1.0, 76 / 255 + 1.402 * 127 / 255)) < 1e-15
    assert abs(got[2] - max(0.0, 76 / 255 + 1.772 * (85 - 128) / 255)) < 1e-15
    assert abs(got[1] - (76 / 255 - (2 * 0.299 * 0.701 / 0.587) * 127 / 255 - (2 * 0.114 * 0.886 / 0.587) * (85 - 128) / 255)) < 1e-15


def test_rgb24_is_a_division_by_255():
    b = np.arange(256, dtype=np.uint8)
    frame = np.repeat(b, 3)          # 256 grey pixels
    img = ref.values32(frame, 1, 256, "rgb24")
    want = torch.from_numpy(b).float().div(255).numpy()
    assert all(np.array_equal(img[c, 0], want) for c in range(3))
    recip = b.astype(np.float32) * np.float32(1.0 / 255.0)
    assert int((recip != want).sum()) == 126          # why the kernel divides


def test_bilinear_weights_on_a_2x2_chroma_plane():
    """c = [[a, b], [c, d]] -> 4 x 4, written out by hand: corners keep their sample (all indices clamped), edges mix two samples
    3 : 1, the inner 2 x 2 mixes four with 9/16, 3/16, 3/16, 1/16."""
    a, b, c, d = 16.0, 240.0, 100.0, 0.0
    up = ref.upsample_codes(np.array([[a, b], [c, d]]), "bilinear")
    want = np.array([
        [a, .75 * a + .25 * b, .25 * a + .75 * b, b],
        [.75 * a + .25 * c, (9 * a + 3 * b + 3 * c + d) / 16, (3 * a + 9 * b + c + 3 * d) / 16, .75 * b + .25 * d],
        [.25 * a + .75 * c, (3 * a + b + 9 * c + 3 * d) / 16, (a + 3 * b + 3 * c + 9 * d) / 16, .25 * b + .75 * d],
        [c, .75 * c + .25 * d, .25 * c + .75 * d, d]])
    assert np.array_equal(up, want)
    assert np.array_equal(ref.upsample_codes(np.array([[a, b], [c, d]]), "bilinear", np.float32), want.astype(np.float32))      # exact in float32
    near = ref.upsample_codes(np.array([[a, b], [c, d]]), "nearest")
    assert np.array_equal(near, [[a, a, b, b], [a, a, b, b], [c, c, d, d], [c, c, d, d]])


def test_bilinear_reference_is_torch_interpolate():
    c = np.random.default_rng(5).integers(0, 256, (9, 13)).astype(np.float64)
    t = torch.nn.functional.interpolate(torch.from_numpy(c)[None, None], scale_factor=2, mode="bilinear", align_corners=False)[0, 0]
    assert np.array_equal(ref.upsample_codes(c, "bilinear"), t.numpy())


# ---- the tolerance of the GPU tests is loose for honest float32 -----------------------------------------------------------------
@pytest.mark.parametrize("matrix,rng", COMBOS)
def test_float32_against_float64_on_a_sixteenth_of_all_triples(matrix, rng):
    k = np.arange(1 << 20, dtype=np.int64)
    t = 16 * k + ((k ^ (k >> 4)) & 15)          # one triple of every 16, every code in every position
    y8, cb8, cr8 = t & 255, (t >> 8) & 255, t >> 16
    assert all(len(np.unique(v)) == 256 for v in (y8, cb8, cr8))
    d = np.abs(ref.rgb_of_codes(y8, cb8, cr8, matrix, rng, np.float32).astype(np.float64) - ref.rgb_of_codes(y8, cb8, cr8, matrix, rng))
    assert d.max() <= 2.0 ** -22, d.max()


@pytest.mark.parametrize("matrix,rng", COMBOS)
@pytest.mark.parametrize("chroma", ["bilinear", "nearest"])
def test_float32_against_float64_on_420_frames(chroma, matrix, rng):
    H = W = 64
    for frame in (ref.random_frame(H, W, "yuv420p", 1), ref.checkerboard_frame(H, W, 2)):
        d = np.abs(ref.values32(frame, H, W, "yuv420p", matrix, rng, chroma).astype(np.float64) - ref.values(frame, H, W, "yuv420p", matrix, rng, chroma))
        assert d.max() <= 2.0 ** -22, d.max()


@pytest.mark.parametrize("matrix,rng", COMBOS)
def test_444_round_trip_of_the_references(matrix, rng):
    """What the GPU round trip relies on: for images in [0.05, 0.95] the bytes of the 4:4:4 nearest conversion survive
    bytes -> float -> bytes, in float64 and in float32, and nothing is clamped on the way."""
    img = np.random.default_rng(11).uniform(0.05, 0.95, (3, 64, 64)).astype(np.float32)
    b = ref_out.convert(img, "yuv444p", matrix, rng, "nearest")
    assert b.size == 12288
    back = ref.values(b, 64, 64, "yuv444p", matrix, rng)
    assert back.min() > 0.0 and back.max() < 1.0          # the clamp did nothing
    assert int((ref_out.convert(back, "yuv444p", matrix, rng, "nearest") != b).sum()) == 0
    back32 = ref.values32(b, 64, 64, "yuv444p", matrix, rng)
    assert back32.min() > 0.0 and back32.max() < 1.0
    assert int((ref_out.quantise32(ref_out.values32(back32, "yuv444p", matrix, rng), "nearest") != b).sum()) == 0


# ---- files ----------------------------------------------------------------------------------------------------------------------
def _write_y4m(path, W, H, T, fmt, seed=0):
    frames = np.stack([ref.random_frame(H, W, fmt.layout, seed + k) for k in range(T)])
    with fo.Y4MWriter(path, W, H, (25, 1), fmt) as sink:
        for fr in frames:
            sink.write(fr)
    return frames


def test_open_video_y4m_header_wins(tmp_path):
    W, H, T = 12, 8, 3
    frames = _write_y4m(tmp_path / "a.y4m", W, H, T, FrameFormat("yuv444p", range="full"))
    hdr, got = fi.open_video(tmp_path / "a.y4m", fmt=FrameFormat("yuv420p", "bt601", "limited"))
    assert (hdr["W"], hdr["H"], hdr["frames"], hdr["frame_bytes"], hdr["fps"]) == (W, H, T, 3 * W * H, (25, 1))
    assert hdr["fmt"] == FrameFormat("yuv444p", "bt601", "full")          # layout and range from the file, the matrix from fmt
    assert got.dtype == np.uint8 and got.shape == (T, 3 * W * H) and np.array_equal(got, frames)
    frames = _write_y4m(tmp_path / "b.y4m", W, H, T, FrameFormat("yuv420p"))
    hdr, got = fi.open_video(tmp_path / "b.y4m", W=999, H=999)
    assert hdr["fmt"] == FrameFormat("yuv420p", "bt709", "limited") and (hdr["W"], hdr["H"]) == (W, H) and np.array_equal(got, frames)
    # a file that does not state its range takes the caller's
    (tmp_path / "c.y4m").write_bytes(f"YUV4MPEG2 W{W} H{H} F30:1 Ip A1:1 C420jpeg\n".encode() + b"FRAME\n" + bytes(frames[0]))
    hdr, got = fi.open_video(tmp_path / "c.y4m", fmt=FrameFormat("yuv420p", "bt709", "full"))
    assert hdr["fmt"].range == "full" and hdr["frames"] == 1 and np.array_equal(got[0], frames[0])
    assert fi.open_video(tmp_path / "c.y4m")[0]["fmt"].range == "limited"


def test_open_video_raw_files_and_refusals(tmp_path):
    W, H, T = 10, 6, 4
    yuv = np.stack([ref.random_frame(H, W, "yuv420p", k) for k in range(T)])
    (tmp_path / "v.yuv").write_bytes(yuv.tobytes())
    hdr, got = fi.open_video(tmp_path / "v.yuv", W, H)
    assert isinstance(got, np.memmap) and got.shape == (T, W * H * 3 // 2) and np.array_equal(got, yuv)
    assert hdr["fmt"] == FrameFormat("yuv420p") and (hdr["W"], hdr["H"], hdr["frames"]) == (W, H, T)
    hdr, got = fi.open_video(tmp_path / "v.yuv", W, H // 2, fmt=FrameFormat("yuv444p", "bt601", "full"))      # the same bytes, read as 4:4:4
    assert hdr["fmt"].layout == "yuv444p" and got.shape == (T, W * H * 3 // 2)
    rgb = np.stack([ref.random_frame(H, W, "rgb24", k) for k in range(T)])
    (tmp_path / "v.rgb").write_bytes(rgb.tobytes())
    hdr, got = fi.open_video(tmp_path / "v.rgb", W, H)
    assert hdr["fmt"].layout == "rgb24" and np.array_equal(got, rgb)
    with pytest.raises(ValueError, match="does not say its size"):
        fi.open_video(tmp_path / "v.yuv")
    (tmp_path / "partial.yuv").write_bytes(yuv.tobytes() + b"\0" * 7)
    with pytest.raises(ValueError, match="not a whole number"):
        fi.open_video(tmp_path / "partial.yuv", W, H)
    (tmp_path / "empty.yuv").write_bytes(b"")
    with pytest.raises(ValueError, match="not a whole number"):
        fi.open_video(tmp_path / "empty.yuv", W, H)
    with pytest.raises(ValueError, match="even"):
        fi.open_video(tmp_path / "v.yuv", 5, 4)
    with pytest.raises(ValueError, match="reads .y4m"):
        fi.open_video(tmp_path / "v.mp4")
    (tmp_path / "bad.y4m").write_bytes(b"YUV4MPEG2 W4 H4 F30:1 C422\nFRAME\n" + b"\0" * 32)
    with pytest.raises(ValueError, match="4:2:0 / 4:4:4"):
        fi.open_video(tmp_path / "bad.y4m")
    (tmp_path / "cut.y4m").write_bytes(b"YUV4MPEG2 W4 H4 F30:1 C420jpeg\nFRAME\n" + b"\0" * 23)
    with pytest.raises(ValueError, match="truncated"):
        fi.open_video(tmp_path / "cut.y4m")


def test_video_file_cube_argument_errors(tmp_path):
    _write_y4m(tmp_path / "a.y4m", 8, 4, 2, FrameFormat("yuv420p"))
    with pytest.raises(ValueError, match="resident"):
        fi.VideoFileCube(tmp_path / "a.y4m", resident="host")
    with pytest.raises(ValueError, match="chroma"):
        fi.VideoFileCube(tmp_path / "a.y4m", chroma="bicubic")
    (tmp_path / "v.yuv").write_bytes(b"\0" * 48)
    with pytest.raises(ValueError, match="does not say its size"):
        fi.VideoFileCube(tmp_path / "v.yuv")
    with pytest.raises(_lib.GsvcError, match="CUDA device"):
        fi.VideoFileCube(tmp_path / "a.y4m", device="cpu")
    with pytest.raises(FileNotFoundError):
        fi.VideoFileCube(tmp_path / "missing.y4m")


def test_frames_from_u8_refuses_before_it_needs_a_gpu():
    with pytest.raises(_lib.GsvcError, match="CPU tensors are not supported"):
        fi.frames_from_u8(torch.zeros(2, 48, dtype=torch.uint8), 4, 4, FrameFormat("rgb24"))
    with pytest.raises(ValueError, match="chroma"):
        fi.frames_from_u8(torch.zeros(2, 48, dtype=torch.uint8), 4, 4, chroma="cubic")
    with pytest.raises(ValueError, match="uint8 tensor"):
        fi.frames_from_u8(np.zeros((2, 48), np.uint8), 4, 4)


# ---- the host-side checks of the C entry point (nothing is launched) --------------------------------------------------------------
def test_c_entry_host_side_checks():
    import __graft_entry__ as g
    import os
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    L = _lib.lib()
    one = (C.c_void_p * 1)(0x1000)
    RGB, P444, P420 = 0, 1, 2

    def call(inp=0x2000, stride=48, n=1, H=4, W=4, layout=RGB, matrix=0, rng=0, chroma=1, images=one):
        return L.gsvc_frames_from_u8(inp, stride, n, H, W, layout, matrix, rng, chroma, images, None)

    for kwargs, message in ((dict(inp=None), b"NULL pointer"), (dict(images=None), b"NULL pointer"), (dict(n=0), b"n must be 1 .. 16"),
                            (dict(n=17), b"n must be 1 .. 16"), (dict(layout=3), b"unknown layout"), (dict(matrix=2), b"unknown matrix"),
                            (dict(rng=-1), b"unknown range"), (dict(chroma=2), b"unknown chroma mode"), (dict(H=0), b"image size"),
                            (dict(W=40000), b"image size"), (dict(layout=P420, H=3, stride=100), b"even H and W"),
                            (dict(layout=P420, W=6, H=5, stride=100), b"even H and W"), (dict(stride=47), b"shorter than a frame"),
                            (dict(layout=P420, stride=23), b"shorter than a frame"), (dict(layout=P444, stride=47), b"shorter than a frame"),
                            (dict(images=(C.c_void_p * 1)(0x1002)), b"not 4-byte aligned"), (dict(images=(C.c_void_p * 1)(0)), b"NULL image pointer")):
        assert call(**kwargs) == -1, kwargs
        assert message in L.gsvc_last_error(), (kwargs, L.gsvc_last_error())
    two = (C.c_void_p * 2)(0x1000, 0x1001)
    assert call(n=2, images=two) == -1 and b"image 1 is not 4-byte aligned" in L.gsvc_last_error()
