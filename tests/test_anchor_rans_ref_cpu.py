"""tests/_anchor_rans_ref.py (the scalar statement of the anchor codec's interleaved rANS, lane count as a parameter) and
gsvc_amd/anchor_codec.py's NumPy coder check each other: the same states and words at the lane counts the codec picks, and each
decodes the other's stream at lane counts it never picks."""
import numpy as np
import pytest

from tests import _anchor_rans_ref as R


def _symbols(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.dirichlet(np.full(40, 0.3))
    return rng.choice(np.arange(1, 241, 6), size=n, p=p).astype(np.int64)


@pytest.mark.parametrize("n", [1, 2, 255, 256, 511, 512, 1000, 5000, 70_000])
def test_reference_writes_the_codecs_stream_at_the_codecs_lanes(n):
    from gsvc_amd import anchor_codec as ac
    sym = _symbols(n, n)
    freq = ac._quantise_freqs(np.bincount(sym, minlength=256).astype(np.int64))
    lanes, states, words = ac._rans_encode(sym, freq)
    assert lanes == max(1, n // 256)
    r_states, r_words = R.encode(sym, freq, lanes)
    assert r_states == states.tolist() and r_words == words.tolist()
    out, err = R.decode(n, freq, lanes, states, words)
    assert err == 0 and out == sym.tolist()
    assert np.array_equal(ac._rans_decode(n, freq, lanes, np.array(r_states, np.uint32), np.array(r_words, np.uint16)), sym)


@pytest.mark.parametrize("lanes,n", [(1, 3000), (2, 5), (63, 62), (64, 129), (65, 65), (1025, 2051), (4097, 4096), (16384, 32769)])
def test_codec_decodes_the_references_stream_at_any_lane_count(lanes, n):
    from gsvc_amd import anchor_codec as ac
    sym = _symbols(n, lanes)
    freq = ac._quantise_freqs(np.bincount(sym, minlength=256).astype(np.int64))
    states, words = R.encode(sym, freq, lanes)
    assert len(states) == lanes and all(v == R.RANS_L for v in states[n:])           # lanes without a symbol stay at 2^16
    assert np.array_equal(ac._rans_decode(n, freq, lanes, np.array(states, np.uint32), np.array(words, np.uint16)), sym)
    out, err = R.decode(n, freq, lanes, states, words)
    assert err == 0 and out == sym.tolist()


def test_reference_decoder_names_each_kind_of_damage():
    sym = _symbols(400, 1)
    freq = np.bincount(sym, minlength=256).astype(np.int64)
    from gsvc_amd import anchor_codec as ac
    freq = ac._quantise_freqs(freq)
    states, words = R.encode(sym, freq, 7)
    assert len(words) > 1
    short = freq.copy()
    short[np.argmax(short)] -= 1
    assert R.decode(400, short, 7, states, words) == ([], R.E_TABLE)
    assert R.decode(400, freq, 7, states, words, n_words=len(words) - 1)[1] == R.E_TRUNCATED
    assert R.decode(400, freq, 7, states, words + [0]) == (sym.tolist(), R.E_END)
    flipped = list(states)
    flipped[3] ^= 1
    assert R.decode(400, freq, 7, flipped, words)[1] in (R.E_TRUNCATED, R.E_END)
    with pytest.raises(ValueError):
        ac._rans_decode(400, freq, 7, np.array(states, np.uint32), np.array(words + [0], np.uint16))
