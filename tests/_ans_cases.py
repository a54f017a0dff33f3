"""Inputs of the direct tests of the attribute coder (gsvc_amd/csrc/ans.hip): the (seg_len, n) shapes, the model builders and the
case table, in one place so that tests/test_ans_cases_cpu.py (conditions on the inputs, from oracle/ans_oracle.py alone) and
tests/test_ans_kernels_gpu.py (the kernels against the oracle) use the same arrays.  Host only, NumPy only.

Shapes.  The decode kernel has one lane per segment, 64 lanes per workgroup and one record group per 64 segments; the encoder's scan
gives each of its 1024 threads ceil(n_seg / 1024) segments; a decode lane keeps ANS_AHEAD = 16 records in flight.  The shapes are the
smallest that stand on both sides of each of these: 64 / 65 / 129 segments (last group full, holding one segment, holding one
segment of one symbol), 1024 / 1025 / 2049 segments (one and two segments per scan thread, ragged), segment lengths 1, 15, 16, 17, 33
and last segments of 1 and 16 symbols around the prefetch depth.
"""
from __future__ import annotations

import functools

import numpy as np

# (seg_len, n)                                 n_seg, last segment
SHAPES = [(16, 1009),                        # 64, last holds 1
          (17, 1088),                        # 64 full
          (15, 961),                         # 65, last holds 1
          (33, 4240),                        # 129, last holds 16
          (4, 4093),                         # 1024, last holds 1
          (3, 3072),                         # 1024 full
          (5, 5121),                         # 1025
          (2, 4097),                         # 2049
          (1, 1100)]                         # one symbol per segment

WIDE = (-262143, 262143)                     # the widest legal alphabet: R = 524 287 = 2^19 - 1, frequency floor F = 1
RANGES = [(-40, 40), (-15000, 15000), (0, 1), WIDE]


def n_segments(seg_len: int, n: int) -> int:
    return (n + seg_len - 1) // seg_len if n > 0 else 0


def mode_of(mu: np.ndarray, smin: int, smax: int) -> np.ndarray:
    """The model's mode as the decoder takes it: clip(floor(mu + 0.5f)) in float32, smin for a NaN."""
    with np.errstate(all="ignore"):
        g = np.floor(np.asarray(mu, np.float32) + np.float32(0.5))
        g = np.where(g == g, np.minimum(np.maximum(g, np.float32(smin)), np.float32(smax)), np.float32(smin))
    return g.astype(np.int64)


def benign(seed: int, n: int, smin: int, smax: int, clamp_sigma: bool = False):
    """The models of the existing byte comparisons (tests/test_codec_gpu.py _oracle_case): sigma in 0.25 .. 6 or at the context
    model's 1e-9 scale clamp, symbols drawn from the model."""
    rng = np.random.default_rng(seed)
    mu = rng.normal(0, min(30.0, smax / 4), n).astype(np.float32)
    sigma = rng.uniform(0.25, 6.0, n).astype(np.float32)
    if clamp_sigma:
        sigma[::3] = np.float32(1e-9 / 0.001)
    sym = np.clip(np.rint(mu.astype(np.float64) + sigma.astype(np.float64) * rng.normal(0, 1, n)), smin, smax).astype(np.int32)
    sym[:2] = [smin, smax][:min(n, 2)]
    return sym, mu, sigma


def extreme(seed: int, n: int, smin: int, smax: int):
    """Every 5th sigma and every 7th mu a value no fitted model holds (zero, infinities, NaN, denormals, the float range's ends, means
    exactly half way between two symbols — with sigma = 0 that is the NaN z of the specification — and beyond the range's ends);
    symbols uniform over the range.  Every symbol keeps its frequency floor, so the specification codes all of it."""
    rng = np.random.default_rng(seed)
    mu = rng.normal(0, min(30.0, smax / 4), n).astype(np.float32)
    sigma = rng.uniform(0.25, 6.0, n).astype(np.float32)
    with np.errstate(all="ignore"):
        bad_sigma = np.array([0.0, np.inf, np.nan, 1e-38, 1e-45, 3e38, 1e-9, 1e4]).astype(np.float32)
        bad_mu = np.array([np.inf, -np.inf, np.nan, 3e38, -3e38, 0.5, -0.5, 1.5, smax - 0.5, smin - 0.5, 1e-40]).astype(np.float32)
    k5, k7 = np.arange(0, n, 5), np.arange(0, n, 7)
    sigma[k5] = bad_sigma[np.arange(k5.size) % bad_sigma.size]
    mu[k7] = bad_mu[np.arange(k7.size) % bad_mu.size]
    sym = rng.integers(smin, smax + 1, n).astype(np.int32)
    return sym, mu, sigma


def unrelated(seed: int, n: int, smin: int, smax: int):
    """Symbols that have nothing to do with their model: mu ~ N(0, R / 10), sigma log-uniform over 0.3 .. R / 10, symbols uniform over
    the range — almost every symbol lies beyond the three the decoder decides by compares, on either side, under narrow and broad
    models alike: the decoder's search (ans_decode_symbol: gallop up / down, the float guess for sigma > 4)."""
    rng = np.random.default_rng(seed)
    R = smax - smin + 1
    mu = rng.normal(0, R / 10, n).astype(np.float32)
    a, b = sorted((np.log(0.3), np.log(R / 10)))            # (R = 2: the interval is 0.2 .. 0.3)
    sigma = np.exp(rng.uniform(a, b, n)).astype(np.float32)
    sym = rng.integers(smin, smax + 1, n).astype(np.int32)
    return sym, mu, sigma


SWEEP_N = 4096
SWEEP_RANGE = (-2, 2)
SWEEP_SEG_LEN = 33                           # 125 segments: a full record group and a partial one


def table_sweep():
    """4096 models with mode 0 whose four record values C(-1), C(0), C(1), C(2) interpolate, between them, EVERY cell of the Phi
    table: mu = 0, sigma_i = float32(1.5 / |z_i|), z_i = -8 + (i + 0.37) / 256, so that s = -1 and s = 2 sit at z = -+|z_i|."""
    i = np.arange(SWEEP_N, dtype=np.float64)
    z = -8.0 + (i + 0.37) / 256.0
    sigma = (1.5 / np.abs(z)).astype(np.float32)
    mu = np.zeros(SWEEP_N, np.float32)
    sym = np.random.default_rng(4096).integers(SWEEP_RANGE[0], SWEEP_RANGE[1] + 1, SWEEP_N).astype(np.int32)
    return sym, mu, sigma


def cell_of(s: int, mu: np.float64, inv_sigma: np.float64):
    """The Phi-table cell C(s) interpolates in, by the specification's own t (oracle/ans_oracle.py docstring); None outside the table."""
    with np.errstate(all="ignore"):
        t = ((np.float64(s) - np.float64(0.5) - mu) * inv_sigma + np.float64(8.0)) * np.float64(256.0)
    return int(t) if t > 0.0 and t < 4096.0 else None


# ---------------------------------------------------------------------------------------------------------------- the case table
# name -> (seg_len, n, smin, smax, builder, builder arguments).  benign and unrelated use every shape (unrelated: every shape with
# the widest range, and once more with one of the other three — 0 .. 1 on the three smallest shapes); extreme uses three.
_BENIGN_RANGES = [(-40, 40, False), (-15000, 15000, False), (0, 255, True), (-2, 2, False), (-15000, 15000, True)]
_SECOND_RANGE = [(0, 1), (-40, 40), (0, 1), (-15000, 15000), (-40, 40), (-15000, 15000), (-40, 40), (-15000, 15000), (0, 1)]
_EXTREME = [((16, 1009), (-40, 40)), ((33, 4240), (-40, 40)), ((5, 5121), (0, 1))]

CASES = {}
for _k, (_seg, _n) in enumerate(SHAPES):
    _lo, _hi, _clamp = _BENIGN_RANGES[_k % len(_BENIGN_RANGES)]
    CASES[f"benign-{_seg}x{_n}"] = (_seg, _n, _lo, _hi, benign, (10 + _k, _n, _lo, _hi, _clamp))
    CASES[f"unrelated-{_seg}x{_n}-wide"] = (_seg, _n, WIDE[0], WIDE[1], unrelated, (30 + _k, _n, WIDE[0], WIDE[1]))
    _lo, _hi = _SECOND_RANGE[_k]
    CASES[f"unrelated-{_seg}x{_n}-{_lo}..{_hi}"] = (_seg, _n, _lo, _hi, unrelated, (50 + _k, _n, _lo, _hi))
for _k, ((_seg, _n), (_lo, _hi)) in enumerate(_EXTREME):
    CASES[f"extreme-{_seg}x{_n}-{_lo}..{_hi}"] = (_seg, _n, _lo, _hi, extreme, (70 + _k, _n, _lo, _hi))
CASES["sweep"] = (SWEEP_SEG_LEN, SWEEP_N, SWEEP_RANGE[0], SWEEP_RANGE[1], table_sweep, ())

BYTE_CASES = [k for k in CASES if k != "sweep"]
RECORD_CASES = [k for k in CASES if k.startswith(("sweep", "extreme", "unrelated"))]


@functools.lru_cache(maxsize=None)
def case(name: str):
    """(seg_len, smin, smax, sym, mu, sigma) of a case; built once, read-only."""
    seg_len, n, smin, smax, build, args = CASES[name]
    sym, mu, sigma = build(*args)
    assert sym.shape == mu.shape == sigma.shape == (n,)
    for a in (sym, mu, sigma):
        a.setflags(write=False)
    return seg_len, smin, smax, sym, mu, sigma


@functools.lru_cache(maxsize=None)
def oracle_stream(name: str) -> bytes:
    """The case's stream as the specification writes it (computed once per process)."""
    from oracle import ans_oracle
    seg_len, smin, smax, sym, mu, sigma = case(name)
    return ans_oracle.encode(sym, mu, sigma, smin, smax, seg_len=seg_len)


# ---------------------------------------------------------------------------------------------------------------- damaged streams
FLIP_N, FLIP_SEG_LEN, FLIP_RANGE = 40, 8, (-20, 20)


@functools.lru_cache(maxsize=None)
def flip_case():
    """The 40-symbol stream whose every payload bit is flipped in turn: (sym, mu, sigma, stream, offset of the payload)."""
    from oracle import ans_oracle
    rng = np.random.default_rng(11)
    mu = rng.normal(0, 6, FLIP_N).astype(np.float32)
    sigma = rng.uniform(0.3, 6, FLIP_N).astype(np.float32)
    sym = np.clip(np.rint(mu + sigma * rng.normal(0, 1, FLIP_N)), *FLIP_RANGE).astype(np.int32)
    stream = ans_oracle.encode(sym, mu, sigma, FLIP_RANGE[0], FLIP_RANGE[1], seg_len=FLIP_SEG_LEN)
    return sym, mu, sigma, stream, ans_oracle.HEADER.size + 4 * n_segments(FLIP_SEG_LEN, FLIP_N)


def flipped(stream: bytes, payload_at: int, bit: int) -> bytes:
    bad = bytearray(stream)
    bad[payload_at + bit // 8] ^= 1 << (bit % 8)
    return bytes(bad)


def resized_segment(stream: bytes, seg: int, delta: int) -> bytes:
    """The stream with segment ``seg`` one byte longer (a zero byte appended behind it, delta = +1) or shorter (its last byte
    removed, -1) and its entry of the size table changed with it: header, size table and payload stay consistent."""
    from oracle import ans_oracle
    assert delta in (1, -1)
    n_seg = ans_oracle.HEADER.unpack_from(stream, 0)[6]
    sizes = np.frombuffer(stream, dtype="<u4", count=n_seg, offset=ans_oracle.HEADER.size).astype(np.int64)
    at = ans_oracle.HEADER.size + 4 * n_seg
    end = at + int(sizes[:seg + 1].sum())
    sizes[seg] += delta
    body = stream[at:end] + b"\0" + stream[end:] if delta > 0 else stream[at:end - 1] + stream[end:]
    return stream[:ans_oracle.HEADER.size] + sizes.astype("<u4").tobytes() + body
