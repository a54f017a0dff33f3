"""Scalar statement of the anchor codec's interleaved rANS (module docstring of gsvc_amd/anchor_codec.py; the stream the kernel
k_anchor_rans_decode of gsvc_amd/csrc/anchor.hip reads), in plain Python integers with the lane count as a PARAMETER — the codec
itself always takes one lane per 256 symbols, which never reaches most of the kernel's lanes-per-thread paths.

  model    static 12-bit frequencies freq[256], sum 4096; cum[s] = freq[0] + .. + freq[s - 1]
  coder    32-bit states x in [2^16, 2^32), 16-bit words.  Symbol i belongs to lane i % lanes; row r is the symbols
           [r lanes, (r + 1) lanes).  Every lane starts at x = 2^16.  Rows are coded from the LAST to the first; in a row, lane
           after lane: if x >= (2^4 << 16) freq[s]: emit x & 0xFFFF, x >>= 16;  then x = (x // freq[s]) << 12 | ... + x % freq[s] + cum[s].
  stream   the lanes' final states, then the words of row 0, row 1, ... — within a row in lane order (the order a decoder that
           walks the rows forwards needs them in).
  decoder  per row, lane after lane: slot = x & 4095, s = the symbol with cum[s] <= slot < cum[s + 1],
           x = freq[s] (x >> 12) + slot - cum[s]; a lane with x < 2^16 takes the next word: x = x << 16 | word.
           Behind the last row every lane is at 2^16 again and every word is used.
"""
PROB_BITS = 12
PROB_SCALE = 1 << PROB_BITS
RANS_L = 1 << 16

# the kernel's error bits
E_TABLE, E_TRUNCATED, E_END = 1, 2, 4


def encode(symbols, freq, lanes: int):
    """-> (states [lanes], words) as lists of Python integers."""
    n = len(symbols)
    freq = [int(f) for f in freq]
    assert sum(freq) == PROB_SCALE and lanes >= 1
    cum = [0] * 257
    for s in range(256):
        cum[s + 1] = cum[s] + freq[s]
    x = [RANS_L] * lanes
    rows = (n + lanes - 1) // lanes
    row_words = []
    for r in range(rows - 1, -1, -1):
        lo = r * lanes
        out = []
        for lane in range(min(lanes, n - lo)):
            s = int(symbols[lo + lane])
            f = freq[s]
            assert f > 0, "symbol without a frequency"
            v = x[lane]
            if v >= ((RANS_L >> PROB_BITS) << 16) * f:
                out.append(v & 0xFFFF)
                v >>= 16
            x[lane] = ((v // f) << PROB_BITS) + (v % f) + cum[s]
        row_words.append(out)
    words = [w for out in reversed(row_words) for w in out]
    return x, words


def decode(n: int, freq, lanes: int, states, words, n_words=None):
    """-> (symbols decoded so far, error bits).  ``n_words``: the word count the decoder is TOLD (default: len(words))."""
    freq = [int(f) for f in freq]
    n_words = len(words) if n_words is None else n_words
    if n == 0:
        return [], 0
    if sum(freq) != PROB_SCALE:
        return [], E_TABLE
    slot2sym = [s for s in range(256) for _ in range(freq[s])]
    cum = [0] * 257
    for s in range(256):
        cum[s + 1] = cum[s] + freq[s]
    x = [int(v) for v in states]
    out = []
    ptr = 0
    for lo in range(0, n, lanes):
        need = []
        for lane in range(min(lanes, n - lo)):
            slot = x[lane] & (PROB_SCALE - 1)
            s = slot2sym[slot]
            out.append(s)
            x[lane] = freq[s] * (x[lane] >> PROB_BITS) + slot - cum[s]
            if x[lane] < RANS_L:
                need.append(lane)
        if ptr + len(need) > n_words:
            return out, E_TRUNCATED
        for lane in need:
            x[lane] = (x[lane] << 16) | int(words[ptr])
            ptr += 1
    bad = ptr != n_words or any(v != RANS_L for v in x)
    return out, E_END if bad else 0
