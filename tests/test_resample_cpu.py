"""Host-side tests of the Lanczos-3 resampler (gsvc_amd/resample.py): the tap tables, the integer arithmetic as
tests/_resample_ref.py restates it against the float64 filter, the DISP section, the new options of the tools and the refusals that
need no device.  Sizes are written W x H."""
import os
import sys

import numpy as np
import pytest

from gsvc_amd import bitstream as B
from gsvc_amd import resample as R
from gsvc_amd.frames_out import FrameFormat

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resample_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
DEPTHS = (8, 10, 12, 16)
_TAPS = {}


def taps(src, dst):
    if (src, dst) not in _TAPS:
        _TAPS[(src, dst)] = R.filter_taps(src, dst)
    return _TAPS[(src, dst)]


def pairs_up_to_40():
    return [(s, d) for s in range(1, 41) for d in range(-(-s // 4), 4 * s + 1)]


# ----------------------------------------------------------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------------------------------------------------------
def test_every_row_sums_to_one_within_24_taps_and_int16_products():
    worst = 0
    for s, d in pairs_up_to_40() + [(1920, 480), (1080, 270)]:
        first, coef, nt = taps(s, d)
        assert first.dtype == np.int32 and first.shape == (d,) and coef.dtype == np.int16 and coef.shape == (d, 24) and 1 <= nt <= 24
        c = coef.astype(np.int64)
        assert (c.sum(axis=1) == 16384).all(), (s, d)
        assert (np.abs(c).sum(axis=1) <= 32767).all(), (s, d)
        assert not c[:, nt:].any()
        for j in range(d):          # the count of the rule, and zeros behind it
            lo, hi, _, _ = R.tap_range(s, d, j)
            assert first[j] == lo and 1 <= hi - lo + 1 <= nt and not c[j, hi - lo + 1:].any(), (s, d, j)
        worst = max(worst, int(np.abs(c).sum(axis=1).max()))
    print("largest sum of |c|:", worst)


def test_same_size_is_one_coefficient_of_16384_at_the_sample_itself():
    for n in (1, 2, 7, 64, 1080):
        first, coef, nt = taps(n, n)
        k = np.arange(24)[None] + first[:, None]
        assert (coef[k == np.arange(n)[:, None]] == 16384).all() and int(np.abs(coef.astype(int)).sum()) == 16384 * n
        assert (first <= np.arange(n)).all() and (np.arange(n) < first + nt).all()


def test_rows_mirror():
    """Row dst - 1 - j is row j mirrored: always in ``first`` and the tap count, and in the coefficients too — with the one exception
    the rule itself makes: a row whose centre lies exactly between two source samples has two equal largest coefficients, step 4 adds
    the rounding residual to the FIRST of them in row j and in its mirror row alike, so there the two rows can differ from mirror images
    in those two centre slots, which hold the same pair in swapped order."""
    exceptions = 0
    for s, d in pairs_up_to_40():
        first, coef, _ = taps(s, d)
        for j in range(d):
            lo, hi, _, _ = R.tap_range(s, d, j)
            n, m = hi - lo + 1, d - 1 - j
            lo2, hi2, _, _ = R.tap_range(s, d, m)
            assert lo2 == s - 1 - hi and hi2 == s - 1 - lo and first[m] == lo2, (s, d, j)
            a, b = coef[j, :n].astype(int), coef[m, :n][::-1].astype(int)
            if not np.array_equal(a, b):
                exceptions += 1
                differ = np.nonzero(a != b)[0].tolist()
                assert n % 2 == 0 and differ == [n // 2 - 1, n // 2] and a[n // 2 - 1] == b[n // 2] and a[n // 2] == b[n // 2 - 1], (s, d, j)
                assert np.array_equal(np.delete(a, differ), np.delete(a[::-1], differ))          # (the row is symmetric apart from the residual)
    print("rows that differ from the mirror image in their two centre slots:", exceptions)
    for s, d in ((16, 8), (8, 16), (1920, 1280), (1080, 2160)):          # the sizes pinned below mirror exactly
        first, coef, nt = taps(s, d)
        for j in range(d):
            n = R.tap_range(s, d, j)[1] - R.tap_range(s, d, j)[0] + 1
            assert np.array_equal(coef[j, :n], coef[d - 1 - j, :n][::-1]), (s, d, j)


def test_pinned_rows():
    first, coef, nt = taps(16, 8)
    assert first[3] == 1 and coef[3, :12].tolist() == [60, 247, -557, -1092, 2220, 7314, 7314, 2220, -1092, -557, 247, 60] and nt == 12
    first, coef, nt = taps(8, 16)
    assert first[6] == 0 and coef[6, :6].tolist() == [121, -1114, 4440, 14628, -2184, 493] and nt == 6
    assert first[7] == 1 and coef[7, :6].tolist() == [493, -2184, 14628, 4440, -1114, 121]
    assert [taps(s, d)[2] for s, d in ((1920, 480), (2160, 1080), (1920, 1280), (1080, 2160))] == [24, 12, 9, 6]


def test_filter_taps_refuses_what_it_cannot_build():
    for s, d in ((0, 4), (4, 0), (17, 4), (4, 17)):
        with pytest.raises(ValueError, match="filter_taps"):
            R.filter_taps(s, d)


# ----------------------------------------------------------------------------------------------------------------------------
# the arithmetic against the float64 filter
# ----------------------------------------------------------------------------------------------------------------------------
SRC_W, SRC_H = 70, 100
SIZES = ((35, 50), (140, 200), (47, 67), (18, 25), (280, 400), (105, 60))
BOUND = {8: 1.0, 10: 1.0, 12: 1.0, 16: 16.0}          # codes; measured in the restatement: 0.514 / 0.587 / 0.822 / 7.54


def inputs(depth, W=SRC_W, H=SRC_H):
    peak = (1 << depth) - 1
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    picture = np.clip(np.rint((0.5 + 0.35 * np.sin(x / 9) * np.cos(y / 7) + 0.1 * np.sin(x / 2.5 + y / 3.1)) * peak), 0, peak).astype(np.int64)
    noise = np.random.default_rng(7).integers(0, peak + 1, (H, W)).astype(np.int64)
    checker = (((np.arange(H)[:, None] + np.arange(W)[None]) & 1) * peak).astype(np.int64)
    return {"picture": picture, "noise": noise, "checkerboard": checker}


@pytest.fixture(scope="module")
def float_matrices():
    """The float64 filter matrices of the sizes used here, built once."""
    out = {}
    for W, H in SIZES:
        out[(SRC_W, W)] = ref.float_matrix(SRC_W, W)
        out[(SRC_H, H)] = ref.float_matrix(SRC_H, H)
    return out


@pytest.mark.parametrize("depth", DEPTHS)
def test_reference_is_the_float64_filter_up_to_rounding(depth, float_matrices):
    peak = (1 << depth) - 1
    worst = 0.0
    for name, plane in inputs(depth).items():
        for W, H in SIZES:
            got = ref.resample_plane(plane, taps(SRC_W, W), taps(SRC_H, H), depth)
            want = np.clip(float_matrices[(SRC_H, H)] @ plane.astype(np.float64) @ float_matrices[(SRC_W, W)].T, 0.0, float(peak))
            assert got.shape == (H, W) and got.min() >= 0 and got.max() <= peak
            err = float(np.abs(got - want).max())
            worst = max(worst, err)
            assert err <= BOUND[depth], (name, W, H, err)
    print(f"depth {depth}: largest difference from the float64 filter {worst:.3f} codes (bound {BOUND[depth]})")


@pytest.mark.parametrize("depth", DEPTHS)
def test_one_to_one_returns_the_input_and_constants_stay_constant(depth):
    peak = (1 << depth) - 1
    for name, plane in inputs(depth).items():
        assert np.array_equal(ref.resample_plane(plane, taps(SRC_W, SRC_W), taps(SRC_H, SRC_H), depth), plane), name
    for value in (0, 1, peak // 3, peak - 1, peak):
        plane = np.full((SRC_H, SRC_W), value, np.int64)
        for W, H in SIZES:
            assert (ref.resample_plane(plane, taps(SRC_W, W), taps(SRC_H, H), depth) == value).all(), (value, W, H)


@pytest.mark.parametrize("depth", DEPTHS)
def test_down_and_up_again_keeps_the_picture(depth):
    """The 96 x 128 picture scaled 2:1 down and back up: 49.6 / 51.0 / 51.1 / 51.1 dB in the restatement; held at 45 dB."""
    peak = (1 << depth) - 1
    W, H = 96, 128
    plane = inputs(depth, W, H)["picture"]
    small = ref.resample_plane(plane, taps(W, W // 2), taps(H, H // 2), depth)
    back = ref.resample_plane(small, taps(W // 2, W), taps(H // 2, H), depth)
    psnr = 10.0 * np.log10(peak ** 2 / np.mean((back - plane).astype(np.float64) ** 2))
    print(f"depth {depth}: {psnr:.2f} dB")
    assert psnr >= 45.0


def test_frames_are_resampled_plane_by_plane():
    """``_resample_ref.resample_frame`` on a 4:2:0 and a 4:4:4 frame: every plane between its own dimensions."""
    rng = np.random.default_rng(1)
    for layout, depth in (("yuv420p", 8), ("yuv444p", 10)):
        H, W, oH, oW = 12, 20, 8, 30
        dims, odims = ref.plane_dims(H, W, layout), ref.plane_dims(oH, oW, layout)
        planes = [rng.integers(0, 1 << depth, d) for d in dims]
        flat = np.concatenate([p.reshape(-1) for p in planes])
        buf = flat.astype("<u2").view(np.uint8) if depth > 8 else flat.astype(np.uint8)
        got = ref.resample_frame(buf, H, W, layout, depth, oH, oW, taps)
        codes = got.view("<u2") if depth > 8 else got
        at = 0
        for p, (h, w), (oh, ow) in zip(planes, dims, odims):
            assert np.array_equal(codes[at:at + oh * ow].reshape(oh, ow), ref.resample_plane(p, taps(w, ow), taps(h, oh), depth))
            at += oh * ow
        assert at == codes.shape[0]


# ----------------------------------------------------------------------------------------------------------------------------
# DISP, the tools, refusals
# ----------------------------------------------------------------------------------------------------------------------------
def _file_sections():
    """The sections of a file that parses (tests/test_bitstream_cpu.py builds such a file from a model; here: the smallest HEAD that
    satisfies ``parse_bitstream``, with no anchors and no slabs)."""
    head = {name: 0 for name in B._HEAD_FIELDS}
    head.update(W=48, H=32, frames=4, fps_num=25, fps_den=1, scale=24.0, x_min=-1.0, y_min=-0.66, z_min=-0.08, threshold=0.3,
                background=[0.0, 0.0, 0.0], raster_low_pass=0.0, voxel_size=0.01, resolutions_list=[4], resolutions_list_2D=[4],
                use_2D=True, ste_binary=True, ste_multistep=False, add_noise=False, Q=1.0, x_bound_min=[-1.0, -1.0, -1.0],
                x_bound_max=[1.0, 1.0, 1.0], prob_masks=0.5, prob_hash=0.5, anchor_interval=[0.1, 0.1, 0.1], anchor_min=[0.0, 0.0, 0.0], slabs=[])
    return [(b"HEAD", B.pack_fields(head)), (b"MLPS", b"m"), (b"ANCH", b"a"), (b"MASK", b""), (b"HASH", b""), (b"SLAB", b"")]


def test_disp_round_trips_and_old_readers_skip_it():
    assert b"DISP" in B.KNOWN_TAGS and b"DISP" not in B.REQUIRED_TAGS
    plain = B.pack_sections(_file_sections())
    bs = B.parse_bitstream(plain)
    assert bs.display is None and bs.coded_size == (48, 32) and bs.display_size == (48, 32)
    blob = B.with_display(plain, (96, 64))
    assert [t for t, _ in B.unpack_sections(blob)][-1] == b"DISP"
    bs = B.parse_bitstream(blob)
    assert bs.display == (96, 64) and bs.display_size == (96, 64) and bs.coded_size == (48, 32) and bs.section_bytes["DISP"] > 0
    assert B.unpack_fields(dict(B.unpack_sections(blob))[b"DISP"], "DISP") == {"display_W": 96, "display_H": 64, "filter": 1}
    assert B.with_display(blob, None) == plain and B.with_display(blob, (96, 64)) == blob
    # a reader with the tag list of before skips the section and sees the coded size only
    old = tuple(t for t in B.KNOWN_TAGS if t != b"DISP")
    assert [t for t, _ in B.unpack_sections(blob, known=old)] == [t for t, _ in B.unpack_sections(plain, known=old)]
    assert dict(B.unpack_sections(blob, known=old))[b"HEAD"] == dict(B.unpack_sections(plain))[b"HEAD"]


def test_disp_refuses_what_it_does_not_know():
    plain = _file_sections()
    for fields, what in (({"display_W": 96, "display_H": 64, "filter": 2}, "unknown filter id 2"),
                         ({"display_W": 96, "display_H": 64}, "filter"), ({"display_W": 96, "display_H": 1, "filter": 1}, "not a picture size"),
                         ({"display_W": 96.0, "display_H": 64, "filter": 1}, "display_W")):
        with pytest.raises(B.BitstreamError, match=what) as e:
            B.parse_bitstream(B.pack_sections(plain + [(b"DISP", B.pack_fields(fields))]))
        assert e.value.section == "DISP"
    with pytest.raises(B.BitstreamError, match="twice"):
        B.parse_bitstream(B.pack_sections(plain + [(b"DISP", B.pack_display(96, 64))] * 2))


def test_delivered_size():
    yuv, rgb = FrameFormat("yuv420p"), FrameFormat("rgb24")
    assert B.delivered_size((48, 32), (96, 64), "display", yuv, "t") == (96, 64)
    assert B.delivered_size((48, 32), None, "display", yuv, "t") == (48, 32)
    assert B.delivered_size((48, 32), (96, 64), "coded", yuv, "t") == (48, 32)
    assert B.delivered_size((48, 32), None, (24, 16), yuv, "t") == (24, 16)
    assert B.delivered_size((48, 32), (96, 64), "display", rgb, "t") == (48, 32) and B.delivered_size((48, 32), None, (24, 16), rgb, "t") == (48, 32)
    for bad, what in (((25, 16), "even"), ((10, 16), "ratio"), ((48, 130), "ratio"), ("half", "size is"), ((48,), "size is")):
        with pytest.raises(ValueError, match=what):
            B.delivered_size((48, 32), None, bad, yuv, "t")
    assert B.delivered_size((48, 32), None, (25, 17), FrameFormat("yuv444p"), "t") == (25, 17)


def test_the_new_options_of_the_tools_parse(capsys):
    import gsvc_decode
    import gsvc_encode
    import scale_video
    assert gsvc_encode.parse_args(["a.y4m", "-o", "a.gsvc"]).coded_size is None
    assert gsvc_encode.parse_args(["a.y4m", "-o", "a.gsvs", "--gop-frames", "8", "--coded-size", "960x540"]).coded_size == (960, 540)
    assert gsvc_decode.parse_args(["a.gsvc", "-o", "a.y4m"]).size == "display"
    assert gsvc_decode.parse_args(["a.gsvc", "-o", "a.y4m", "--size", "coded"]).size == "coded"
    assert gsvc_decode.parse_args(["a.gsvc", "-o", "a.y4m", "--size", "480X270"]).size == (480, 270)
    args = scale_video.parse_args(["a.y4m", "b.y4m", "--size", "64x48", "--video-size", "32x24"])
    assert args.size == (64, 48) and args.video_size == (32, 24)
    for tool, argv in ((gsvc_encode, ["a.y4m", "-o", "a.gsvc", "--coded-size", "960"]), (gsvc_encode, ["a.y4m", "-o", "a.gsvc", "--coded-size", "0x4"]),
                       (gsvc_encode, ["a.y4m", "-o", "a.gsvc", "--coded-size", "96x64", "--film-grain"]),
                       (gsvc_encode, ["a.y4m", "-o", "a.gsvc", "--coded-size", "96x64", "--flow-dir", "flows"]),
                       (gsvc_decode, ["a.gsvc", "-o", "a.y4m", "--size", "large"]), (scale_video, ["a.y4m", "b.y4m"]),
                       (scale_video, ["a.y4m", "b.png", "--size", "64x48"])):
        with pytest.raises(SystemExit):
            tool.parse_args(argv)
    capsys.readouterr()


def test_refusals_that_need_no_device():
    import torch
    frames = torch.zeros((1, 3 * 16 * 16), dtype=torch.uint8)
    for fmt, size, what in ((FrameFormat("rgb24"), (8, 8), "rgb24"), (FrameFormat("yuv420p"), (9, 8), "even"),
                            (FrameFormat("yuv444p"), (8, 3), "ratio"), (FrameFormat("yuv444p"), (65, 8), "ratio"),
                            (FrameFormat("yuv444p"), (1, 8), "at least 2")):
        with pytest.raises(ValueError, match=what):
            R.resample_frames(frames, 16, 16, fmt, size[0], size[1])
    with pytest.raises(ValueError, match="at least 2"):
        R.check_sizes(1, 16, 2, 16, FrameFormat("yuv444p"), "t")
    with pytest.raises(ValueError, match="even"):
        R.check_sizes(16, 18, 16, 9 * 2 + 1, FrameFormat("yuv420p"), "t")
