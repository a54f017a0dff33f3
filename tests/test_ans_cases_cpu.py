"""Conditions on the inputs of tests/test_ans_kernels_gpu.py, asserted from the specification (oracle/ans_oracle.py) alone: the
models reach the code paths they are there for, and the strict end-of-segment rule refuses every single-bit damage of a stream."""
import numpy as np
import pytest

from tests import _ans_cases as K


def test_shapes_stand_on_both_sides_of_every_boundary():
    segs = {(s, n): (K.n_segments(s, n), n - (K.n_segments(s, n) - 1) * s) for s, n in K.SHAPES}
    assert segs == {(16, 1009): (64, 1), (17, 1088): (64, 17), (15, 961): (65, 1), (33, 4240): (129, 16), (4, 4093): (1024, 1),
                    (3, 3072): (1024, 3), (5, 5121): (1025, 1), (2, 4097): (2049, 1), (1, 1100): (1100, 1)}
    used = {}
    for name in K.BYTE_CASES:
        seg_len, smin, smax, sym, mu, sigma = K.case(name)
        used.setdefault(name.split("-")[0], set()).add((seg_len, sym.size))
        assert sym.min() >= smin and sym.max() <= smax and smax - smin + 1 < (1 << 19)
    assert used["benign"] == used["unrelated"] == set(K.SHAPES) and len(used["extreme"]) == 3
    from oracle import ans_oracle
    assert K.WIDE[1] - K.WIDE[0] + 1 == 524287 and ans_oracle.floor_of(524287) == 1


def test_unrelated_symbols_drive_the_decoders_search_on_both_sides_and_both_model_widths():
    """At least 90 % of the `unrelated` symbols lie two or more from the mode (the decoder decides mode - 1 .. mode + 1 by compares
    and searches for the rest), and each of the four classes of those — above / below the mode, sigma <= 4 (plain gallop) / sigma > 4
    (float guess first) — holds at least 10 % of them."""
    far = total = 0
    classes = np.zeros((2, 2), np.int64)
    for name in K.BYTE_CASES:
        if not name.startswith("unrelated"):
            continue
        seg_len, smin, smax, sym, mu, sigma = K.case(name)
        d = sym.astype(np.int64) - K.mode_of(mu, smin, smax)
        m = np.abs(d) >= 2
        total += sym.size
        far += int(m.sum())
        for above in (0, 1):
            for broad in (0, 1):
                classes[above, broad] += int((m & ((d > 0) == bool(above)) & ((sigma > 4.0) == bool(broad))).sum())
        if (smin, smax) == K.WIDE:
            assert m.mean() >= 0.999, (name, m.mean())
    print(f"unrelated: {far} of {total} symbols two or more from the mode; classes {classes.tolist()}")
    assert far >= 0.9 * total, (far, total)
    assert (classes >= 0.1 * far).all(), (classes, far)


def test_extreme_models_hold_every_listed_value_and_clamped_modes():
    for name in K.BYTE_CASES:
        if not name.startswith("extreme"):
            continue
        seg_len, smin, smax, sym, mu, sigma = K.case(name)
        assert np.isnan(sigma).any() and np.isinf(sigma).any() and (sigma == 0).any() and np.isnan(mu).any()
        assert (mu == np.inf).any() and (mu == -np.inf).any()
        tiny = sigma[(sigma > 0) & (sigma < np.finfo(np.float32).tiny)]
        assert tiny.size and (mu[(mu > 0) & (mu < np.finfo(np.float32).tiny)]).size           # denormals survive as float32
        mode = K.mode_of(mu, smin, smax)
        with np.errstate(all="ignore"):
            assert ((mode == smin) & (mu < smin)).any() and ((mode == smax) & (mu > smax)).any()      # modes clamped at both ends
        assert set(np.unique(sym)) >= {smin, smax}


def test_table_sweep_interpolates_every_cell_of_the_phi_table():
    from oracle import ans_oracle
    seg_len, smin, smax, sym, mu, sigma = K.case("sweep")
    assert smin <= -2 and smax >= 2 and (K.mode_of(mu, smin, smax) == 0).all()
    m64, inv = ans_oracle._model(mu, sigma)
    cells = set()
    for i in range(sym.size):
        for s in (-1, 0, 1, 2):
            c = K.cell_of(s, m64[i], inv[i])
            if c is not None:
                cells.add(c)
    assert cells == set(range(4096)), len(cells)


@pytest.mark.parametrize("name", ["extreme-16x1009--40..40", "extreme-5x5121-0..1", "unrelated-15x961-wide", "sweep"])
def test_the_specification_codes_these_models(name):
    from oracle import ans_oracle
    seg_len, smin, smax, sym, mu, sigma = K.case(name)
    assert np.array_equal(ans_oracle.decode(K.oracle_stream(name), mu, sigma), sym)


def test_end_rule_refuses_every_single_bit_flip_of_a_payload():
    """Without the end rule (no byte left, state 2^23 again behind a segment's last symbol) 115 of these 264 flips decode to other
    symbols with no error; with it every one is refused."""
    from oracle import ans_oracle
    sym, mu, sigma, stream, at = K.flip_case()
    assert np.array_equal(ans_oracle.decode(stream, mu, sigma), sym)
    bits = 8 * (len(stream) - at)
    assert bits == 264
    refused = 0
    for b in range(bits):
        try:
            ans_oracle.decode(K.flipped(stream, at, b), mu, sigma)
        except ValueError:
            refused += 1
    assert refused == bits, (refused, bits)


def test_resized_segments_are_refused():
    from oracle import ans_oracle
    sym, mu, sigma, stream, at = K.flip_case()
    for seg in range(K.n_segments(K.FLIP_SEG_LEN, K.FLIP_N)):
        for delta in (1, -1):
            bad = K.resized_segment(stream, seg, delta)
            assert len(bad) == len(stream) + delta
            with pytest.raises(ValueError):
                ans_oracle.decode(bad, mu, sigma)
