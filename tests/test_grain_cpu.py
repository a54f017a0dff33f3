"""CPU tests of the film-grain model (gsvc_amd/grain.py): the GRAN payload bit for bit and every way it can be
damaged, the section inside a bitstream file, the statistics of the reference noise (tests/_grain_ref.py) against the formulas of the
module's docstring, and the closed loop flat patches + grain -> statistics -> ``fit_grain`` -> the parameters put in."""
import math
import struct

import numpy as np
import pytest

from gsvc_amd import bitstream as B
from gsvc_amd import grain as G
from gsvc_amd.frames_out import FrameFormat
from tests import _grain_ref as ref
from tests.test_bitstream_cpu import _file


def _params(**over):
    rng = np.random.default_rng(3)
    kw = dict(seed=0xFEDCBA9876543210, scale=tuple(tuple(int(v) for v in rng.integers(0, 65536, 17)) for _ in range(3)), kx=(-32, 0, 32),
              ky=(7, -9, 32), source=FrameFormat("yuv420p", "bt601", "full", depth=10))
    kw.update(over)
    return G.GrainParams(**kw)


# ---- the payload ----------------------------------------------------------------------------------------------------------------------
def test_pack_unpack_round_trip_bit_for_bit():
    p = _params()
    blob = p.pack()
    assert len(blob) == 122 and blob[0] == 1 and struct.unpack_from("<Q", blob, 1)[0] == p.seed
    assert tuple(blob[9:14]) == (2, 10, 1, 1, 1)                       # yuv420p, 10 bits, bt601, full, nearest
    assert struct.unpack_from("<51H", blob, 14) == tuple(v for row in p.scale for v in row)
    assert struct.unpack_from("<6b", blob, 116) == (-32, 0, 32, 7, -9, 32)
    back = G.GrainParams.unpack(blob)
    assert back == G.GrainParams(**dict(p.__dict__, source=FrameFormat("yuv420p", "bt601", "full", "nearest", 10))) and back.pack() == blob
    assert back.source.depth == 10 and back.source.range == "full" and not back.is_zero
    assert G.GrainParams(seed=1, scale=((0,) * 17,) * 3).is_zero
    for bad in (dict(seed=-1), dict(seed=1 << 64), dict(kx=(0, 33, 0)), dict(ky=(0, 0, -33)), dict(scale=((0,) * 17,) * 2),
                dict(scale=((0,) * 16,) * 3), dict(scale=((70000,) + (0,) * 16,) * 3), dict(source=FrameFormat("rgb24"))):
        with pytest.raises(ValueError):
            _params(**bad)


def test_every_truncation_and_out_of_range_field_is_named_gran():
    blob = _params().pack()
    for cut in list(range(len(blob))) + [len(blob) + 1]:
        with pytest.raises(B.BitstreamError) as e:
            G.GrainParams.unpack((blob + b"\0")[:cut])
        assert e.value.section == "GRAN" and "GRAN" in str(e.value), cut
    # offsets: 0 version, 9 layout, 10 depth, 11 matrix, 12 range, 13 rounding, 116 .. 118 kx, 119 .. 121 ky
    for at, value in ((0, 0), (0, 2), (9, 0), (9, 3), (10, 9), (10, 0), (11, 2), (12, 2), (13, 2), (116, 33), (118, 256 - 33), (119, 127), (121, 128)):
        edited = bytearray(blob)
        edited[at] = value
        with pytest.raises(B.BitstreamError) as e:
            G.GrainParams.unpack(bytes(edited))
        assert e.value.section == "GRAN", (at, value)


# ---- the section in a file -------------------------------------------------------------------------------------------------------------
def test_a_file_with_gran_parses_and_without_it_is_the_same_file_otherwise():
    plain = _file()[0]
    p = _params()
    blob = B.with_grain(plain, p)
    assert [t for t, _ in B.unpack_sections(blob)] == [b"HEAD", b"MLPS", b"ANCH", b"MASK", b"HASH", b"SLAB", b"PHSH", b"GRAN"]
    assert B.KNOWN_TAGS[-1] == b"GRAN" and B.REQUIRED_TAGS == (b"HEAD", b"MLPS", b"ANCH", b"MASK", b"HASH", b"SLAB") and B.VERSION == 1
    bs = B.parse_bitstream(blob)
    assert bs.grain == G.GrainParams.unpack(p.pack()) and bs.section_bytes["GRAN"] == 122
    assert B.with_grain(blob, None) == plain and B.with_grain(blob, p) == blob          # removed; set again: one section
    without = B.parse_bitstream(B.with_grain(blob, None))
    assert without.grain is None and B.parse_bitstream(plain).grain is None
    for name in ("header", "mlp_bytes", "hash_format"):
        assert str(getattr(without, name)) == str(getattr(bs, name)), name
    assert np.array_equal(without.hashes, bs.hashes) and without.pack.anchor_stream == bs.pack.anchor_stream and without.pack.feat == bs.pack.feat
    assert {k: v for k, v in bs.section_bytes.items() if k != "GRAN"} == without.section_bytes
    # a decoder that does not know the tag (its KNOWN_TAGS end at PHSH) reads the same sections
    assert B.unpack_sections(blob, known=B.KNOWN_TAGS[:7]) == B.unpack_sections(plain, known=B.KNOWN_TAGS[:7])
    # with_hashes keeps GRAN, bitstream_bytes writes it
    fmt, h = _file()[4:]
    again = B.parse_bitstream(B.with_hashes(blob, fmt, h[::-1].copy()))
    assert again.grain == bs.grain and np.array_equal(again.hashes, h[::-1])
    assert B.parse_bitstream(B.with_hashes(blob, None, None)).grain == bs.grain
    # a damaged section is named
    entries = B.unpack_sections(blob)
    with pytest.raises(B.BitstreamError) as e:
        B.parse_bitstream(B.pack_sections(entries[:-1] + [(b"GRAN", p.pack()[:-1])]))
    assert e.value.section == "GRAN"
    with pytest.raises(B.BitstreamError) as e:
        B.parse_bitstream(B.pack_sections(entries + [(b"GRAN", p.pack())]))
    assert e.value.section == "GRAN"


def test_rgb24_and_bad_arguments_are_refused_before_anything_runs():
    import torch
    p = _params()
    buf = torch.zeros(64 * 48 * 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="rgb24"):
        G.apply_grain(buf, 48, 64, FrameFormat("rgb24"), p)
    with pytest.raises(ValueError, match="rgb24"):
        G.grain_stats(buf, buf, 48, 64, FrameFormat("rgb24"))
    with pytest.raises(ValueError):
        G.fit_grain(np.zeros((3, 15, 6), np.int64), 1)
    zero = G.fit_grain(np.zeros((3, 16, 6), np.int64), 5)
    assert zero.is_zero and zero.kx == (0, 0, 0) and zero.seed == 5


# ---- the reference noise against the formulas ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kx,ky", [(0, 0), (16, 16), (32, 0), (-16, 8)])
def test_reference_noise_statistics_match_the_formulas(kx, ky):
    """256 x 256 samples of n.  Tolerances: six standard errors, from the sample count N and the model's own correlations rho (lags 0, 1, 2
    each way, separable): the mean of N correlated samples has variance var sum(rho) / N; the sample variance var^2 2 sum(rho^2) / N (a
    Gaussian bound: the Irwin-Hall kurtosis is below it); a sample correlation at most sum(rho^2) / N (Bartlett's formula is below it for
    these filters)."""
    side = 256
    n = ref.filtered(0xABCDEF, 11, 1, side, side, kx, ky).astype(np.float64)
    N = side * side
    g = ref.white(0xABCDEF, 11, 1, -1, side + 1, -1, side + 1)
    assert g.min() >= -510 and g.max() <= 510 and abs(g.astype(np.float64).var() / 21845.0 - 1) < 6 * math.sqrt(2.0 / g.size)
    var = ref.noise_variance(kx, ky)
    assert var == G.noise_variance(kx, ky) and ref.lag1(kx) == G.lag1(kx)
    rho = lambda k: (1.0, ref.lag1(k), ref.lag2(k))          # noqa: E731
    sum_rho = (1 + 2 * rho(kx)[1] + 2 * rho(kx)[2]) * (1 + 2 * rho(ky)[1] + 2 * rho(ky)[2])
    sum_rho2 = (1 + 2 * rho(kx)[1] ** 2 + 2 * rho(kx)[2] ** 2) * (1 + 2 * rho(ky)[1] ** 2 + 2 * rho(ky)[2] ** 2)
    assert abs(n.mean()) <= 6 * math.sqrt(var * sum_rho / N)
    assert abs(n.var() / var - 1) <= 6 * math.sqrt(2 * sum_rho2 / N)
    tol = 6 * math.sqrt(sum_rho2 / N)
    assert abs(np.mean(n[:, 1:] * n[:, :-1]) / n.var() - ref.lag1(kx)) <= tol
    assert abs(np.mean(n[1:] * n[:-1]) / n.var() - ref.lag1(ky)) <= tol
    if (kx, ky) == (16, 16):
        assert abs(ref.lag1(16) - 0.444) < 1e-3 and abs(ref.lag1(32) - 0.667) < 1e-3


def test_noise_depends_on_seed_frame_plane_and_position_only():
    a = ref.white(5, 3, 0, -1, 20, -1, 40)
    assert np.array_equal(ref.white(5, 3, 0, 4, 9, 6, 31), a[5:10, 7:32])          # any window of it: no tile, no origin
    for other in (ref.white(6, 3, 0, -1, 20, -1, 40), ref.white(5, 4, 0, -1, 20, -1, 40), ref.white(5, 3, 1, -1, 20, -1, 40)):
        assert not np.array_equal(other, a)


# ---- the closed loop -----------------------------------------------------------------------------------------------------------------
def test_closed_loop_returns_the_parameters_put_in():
    """Flat patches + reference grain against the flat patches -> ``stats_ref`` -> ``fit_grain``.  Measured here on the CPU for
    ``_grain_ref.closed_loop_case()`` (luma 256 blocks per bin, chroma 64): every tap comes back exactly, the strengths within 2.567 %
    (``_grain_ref.CLOSED_LOOP_MEASURED``); held with a margin of 2 x."""
    c = ref.closed_loop_case()
    src = ref.apply_ref(c["dec"], c["H"], c["W"], c["layout"], c["depth"], c["range"], c["seed"], c["scale"], c["kx"], c["ky"], c["frame_ids"])
    stats = ref.stats_ref(src, c["dec"], c["H"], c["W"], c["layout"], c["depth"], 0, 32)
    assert stats[0, :, 0].tolist() == [256] * 16 and stats[1, :, 0].tolist() == stats[2, :, 0].tolist() == [64] * 16
    got = G.fit_grain(stats, seed=9, source=FrameFormat("yuv420p", range="full"))
    rel, tap = ref.recovery_error(c, got.scale, got.kx, got.ky)
    print(f"closed loop: strengths within {rel:.5f}, taps within {tap}")
    assert rel <= ref.CLOSED_LOOP_BOUND[0] and tap <= ref.CLOSED_LOOP_BOUND[1]
    assert got.seed == 9 and got.source.range == "full"
    # the library's fit is the reference's
    scale, kx, ky = ref.fit_ref(stats)
    assert list(got.kx) == kx and list(got.ky) == ky and max(abs(a - b) for r1, r2 in zip(got.scale, scale) for a, b in zip(r1, r2)) <= 1
    # gain scales the strengths; bins below min_blocks take their neighbours'; a plane without blocks is zero
    double = G.fit_grain(stats, 9, gain=2.0)
    assert max(abs(d - 2 * s) for r1, r2 in zip(double.scale, got.scale) for d, s in zip(r1, r2)) <= 1
    few = stats.copy()
    few[0, 5:9, :] = 0
    few[2] = 0
    holes = G.fit_grain(few, 9)
    assert holes.scale[2] == (0,) * 17 and holes.kx[2] == holes.ky[2] == 0
    lo, hi = holes.scale[0][4], holes.scale[0][10]
    assert all(min(lo, hi) - 1 <= v <= max(lo, hi) + 1 for v in holes.scale[0][5:10]) and holes.scale[0][7] not in (0, 65535)
    assert G.blocks_used(stats) == [4096, 1024, 1024]


def test_the_tools_take_the_film_grain_flags(capsys):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fit_synthetic
    import gsvc_decode
    import gsvc_encode
    for tool, argv in ((gsvc_encode, ["clip.y4m", "-o", "clip.gsvc", "--film-grain-gain", "2"]),
                       (gsvc_encode, ["clip.y4m", "-o", "clip.gsvc", "--film-grain-seed", "7"]), (fit_synthetic, ["--film-grain"])):
        with pytest.raises(SystemExit):
            tool.main(argv)
        assert "--film-grain" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        gsvc_decode.main(["--help"])
    assert "--no-film-grain" in capsys.readouterr().out
