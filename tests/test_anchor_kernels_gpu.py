"""The kernels of the anchor-geometry decoder (gsvc_amd/csrc/anchor.hip) called directly through the C ABI and compared for
equality with plain Python: k_anchor_rans_decode against the scalar statement tests/_anchor_rans_ref.py at every lanes-per-thread
count from 1 to 16 (the codec's own streams stop at 5), with fewer symbols than lanes, with the zero-word level, with each error
bit; k_popcount_u8 / k_octree_expand / k_demorton against loops over bits."""
import functools

import numpy as np
import pytest
import torch

from tests import _anchor_rans_ref as R

pytestmark = pytest.mark.gpu

SENT = 0xEE
GUARD = 67                       # bytes of sentinel on either side of every output (odd: the outputs are not aligned)

# 1024 threads: lanes / thread = 1 (.. 1024), 2 (1025 .. 2048), 3 (2049), 5 (4097), 16 (15361 .. 16384); the wave (64) and
# workgroup (1024) boundaries +- 1
LANES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 15361, 16383, 16384]
SHAPES = [(lanes, n) for lanes in LANES for n in (lanes - 1, lanes, 2 * lanes + 1) if n >= 1] + [(1, 3000)]


def _table(name):
    f = np.zeros(256, np.int64)
    if name == "skewed":
        f[3], f[77], f[255] = 3000, 1000, 96
    elif name == "flat":
        f[:] = 16
    elif name == "single":
        f[200] = 4096
    elif name == "rare":
        f[9], f[10] = 4095, 1
    elif name == "geometric":                              # 1 .. 12 bits per symbol: which lanes take a word differs from row to row
        f[20:32] = [2048 >> k for k in range(12)]
        f[40] = 1
    assert f.sum() == 4096
    return f


@functools.lru_cache(maxsize=None)
def _level(table: str, lanes: int, n: int):
    """One level coded by the reference: dict(freq, states, words, sym, lanes, n)."""
    freq = _table(table)
    rng = np.random.default_rng(lanes * 7 + n)
    # (geometric: every present symbol equally often, not by its frequency — any symbol with a frequency can be coded)
    sym = rng.choice(np.flatnonzero(freq), size=n) if table == "geometric" else rng.choice(256, size=n, p=freq / 4096.0)
    if table == "rare":
        sym[n // 2] = 10                                   # the frequency-1 symbol is there
    states, words = R.encode(sym, freq, lanes)
    out, err = R.decode(n, freq, lanes, states, words)
    assert err == 0 and out == sym.tolist()
    if table == "single":
        assert not words and all(v == R.RANS_L for v in states)
    return dict(freq=freq.astype(np.uint16), states=np.array(states, np.uint32), words=np.array(words, np.uint16), sym=sym.astype(np.uint8),
                lanes=lanes, n=n)


def _launch(levels):
    """One gsvc_anchor_rans_decode call.  A level is a dict as _level returns it, optionally with ``n_words`` (the count the kernel
    is told) and ``null`` (all pointers NULL).  Returns (return code, error word, per-level output bytes, guards untouched)."""
    from gsvc_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda")
    sections, size = [], 0

    def put(arr):
        nonlocal size
        off = size
        sections.append((off, arr))
        size = (off + arr.nbytes + 15) // 16 * 16
        return off
    offs = [None if lv.get("null") else (put(lv["freq"]), put(lv["states"]), put(lv["words"]) if lv["words"].size else None) for lv in levels]
    blob = np.zeros(max(size, 16), np.uint8)
    for off, arr in sections:
        blob[off:off + arr.nbytes] = arr.view(np.uint8).reshape(-1)
    g = torch.from_numpy(blob).to(dev)
    out_at, pos = [], GUARD
    for lv in levels:
        out_at.append(pos)
        pos += lv["n"] + GUARD
    out = torch.full((pos,), SENT, dtype=torch.uint8, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    descs = (_lib.AnchorLevelC * max(len(levels), 1))()
    for d, lv, o, at in zip(descs, levels, offs, out_at):
        d.n, d.lanes = lv["n"], lv["lanes"]
        d.n_words = lv.get("n_words", 0 if lv.get("null") else int(lv["words"].size))
        if o is not None:
            d.freq, d.states, d.out = g.data_ptr() + o[0], g.data_ptr() + o[1], out.data_ptr() + at
            d.words = None if o[2] is None else g.data_ptr() + o[2]
    rc = L.gsvc_anchor_rans_decode(descs, len(levels), _lib.ptr(err), _lib.current_stream(dev))
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    outs = [host[at:at + lv["n"]] for lv, at in zip(levels, out_at)]
    guards = all((host[at - GUARD:at] == SENT).all() for at in out_at) and (host[pos - GUARD:] == SENT).all()
    return rc, int(err.item()), outs, guards


@pytest.mark.parametrize("table", ["skewed", "flat", "single", "rare"])
def test_rans_decode_at_every_lanes_per_thread_count(table):
    levels = [_level(table, lanes, n) for lanes, n in SHAPES]
    assert len(levels) == 45
    for k in range(0, len(levels), 16):
        batch = levels[k:k + 16]
        rc, err, outs, guards = _launch(batch)
        assert rc == 0 and err == 0
        for lv, o in zip(batch, outs):
            assert np.array_equal(o, lv["sym"]), (table, lv["lanes"], lv["n"], int(np.flatnonzero(o != lv["sym"])[0]))
        assert guards


def test_rans_decode_with_irregular_renormalisation():
    """Symbols of 1 .. 12 bits in up to 7 rows: the lanes that renormalise change from row to row, so a word's position in the
    stream is a different workgroup scan every time (under the other tables a row's lanes renormalise all together or not at all)."""
    shapes = SHAPES + [(lanes, 6 * lanes + 5) for lanes in (64, 65, 1024, 1025, 2049, 4097, 15361, 16384)]
    levels = [_level("geometric", lanes, n) for lanes, n in shapes]
    mixed = 0
    for k in range(0, len(levels), 16):
        batch = levels[k:k + 16]
        rc, err, outs, guards = _launch(batch)
        assert rc == 0 and err == 0 and guards
        for lv, o in zip(batch, outs):
            assert np.array_equal(o, lv["sym"]), (lv["lanes"], lv["n"], int(np.flatnonzero(o != lv["sym"])[0]))
            mixed += 0 < lv["words"].size < lv["n"]
    assert mixed == sum(n > lanes for lanes, n in shapes) == 24          # every level of two rows or more (one row emits nothing)


def test_sixteen_levels_in_one_launch_one_of_them_empty():
    tables = ["skewed", "flat", "single", "rare"]
    pick = [(16384, 32769), (1, 3000), (65, 64), (2049, 2049), (15361, 15360), (1024, 2049), (2, 5), (4097, 8195), (63, 127), (2047, 2046),
            (16383, 16383), (64, 64), (1025, 2051), (2048, 4097), (1023, 1022)]
    levels = [_level(tables[k % 4], lanes, n) for k, (lanes, n) in enumerate(pick)]
    levels.insert(6, dict(n=0, lanes=1, null=True))
    assert len(levels) == 16 and len({lv["lanes"] for lv in levels}) >= 15
    rc, err, outs, guards = _launch(levels)
    assert rc == 0 and err == 0 and guards
    for lv, o in zip(levels, outs):
        assert lv["n"] == 0 or np.array_equal(o, lv["sym"]), (lv["lanes"], lv["n"])


def _damaged(kind):
    """(level, the reference's verdict on it: (symbols, error bits))"""
    if kind == "table":
        lv = dict(_level("skewed", 65, 131))
        lv["freq"] = lv["freq"].copy()
        lv["freq"][3] -= 1                                                    # sums to 4095
    elif kind == "truncated":
        lv = dict(_level("flat", 1025, 2051))
        lv["n_words"] = int(lv["words"].size) - 1                             # told one word fewer; the buffer itself is complete
    elif kind == "word too many":
        lv = dict(_level("flat", 2049, 4099))
        lv["words"] = np.concatenate([lv["words"], np.array([0x1234], np.uint16)])
    elif kind == "state":
        lv = dict(_level("skewed", 65, 131))
        lv["states"] = lv["states"].copy()
        lv["states"][5] ^= 1
    elif kind == "idle state":                                                # a lane that holds no symbol must still be at 2^16
        lv = dict(_level("skewed", 64, 63))
        lv["states"] = lv["states"].copy()
        lv["states"][63] ^= 1
    return lv, R.decode(lv["n"], lv["freq"], lv["lanes"], lv["states"], lv["words"], n_words=lv.get("n_words"))


@pytest.mark.parametrize("kind,bit", [("table", 1), ("truncated", 2), ("word too many", 4), ("state", 4), ("idle state", 4)])
def test_each_error_bit_with_the_other_levels_still_decoded(kind, bit):
    bad, (ref_sym, ref_err) = _damaged(kind)
    assert ref_err == bit
    good = [_level("rare", 16384, 32769), _level("skewed", 2, 5)]
    rc, err, outs, guards = _launch([good[0], bad, good[1]])
    assert rc == 0 and err == bit and guards
    assert np.array_equal(outs[0], good[0]["sym"]) and np.array_equal(outs[2], good[1]["sym"])
    if bit == 1:
        assert (outs[1] == SENT).all()                                        # refused before anything is written
    elif bit == 4:
        assert outs[1].tolist() == ref_sym                                    # every row was decoded; only the end check failed


def test_error_bits_of_several_levels_are_ored():
    kinds = ["table", "truncated", "word too many", "state"]
    good = _level("flat", 4097, 8195)
    levels = [good] + [_damaged(k)[0] for k in kinds] + [good]
    rc, err, outs, guards = _launch(levels)
    assert rc == 0 and err == 7 and guards
    assert np.array_equal(outs[0], good["sym"]) and np.array_equal(outs[-1], good["sym"])


def test_host_refuses_bad_arguments_without_a_launch():
    ok = _level("skewed", 2, 5)
    assert _launch([ok])[:2] == (0, 0)
    for levels in ([], [ok] * 17, [dict(ok, lanes=0)], [dict(ok, lanes=16385)], [dict(n=5, lanes=2, null=True)]):
        rc, err, outs, guards = _launch(levels)
        assert rc != 0 and err == 0 and guards
        assert all((o == SENT).all() for o in outs)


# ---------------------------------------------------------------------------------------------------------------- octree kernels
def _popcount(m):
    return sum((int(m) >> c) & 1 for c in range(8))


def _masks(n, seed, with_zero=False):
    rng = np.random.default_rng(seed)
    every = np.arange(0 if with_zero else 1, 256)
    m = np.concatenate([rng.permutation(every), rng.integers(1, 256, max(0, n - every.size))])[:n] if n > 1 else np.array([0x96])
    return m.astype(np.uint8)


def _expand(nodes, occ, incl, capacity, size):
    """gsvc_octree_expand into a sentinel-filled buffer of ``size`` entries: (error word, buffer)."""
    from gsvc_amd import _lib
    dev = torch.device("cuda")
    out = torch.full((size,), -1, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    nodes_d = None if nodes is None else torch.from_numpy(nodes).to(dev)
    occ_d, incl_d = torch.from_numpy(occ).to(dev), torch.from_numpy(incl).to(dev)
    _lib.check(_lib.lib().gsvc_octree_expand(_lib.ptr(nodes_d), _lib.ptr(occ_d), _lib.ptr(incl_d), occ.size, capacity, _lib.ptr(out),
                                             _lib.ptr(err), _lib.current_stream(dev)), "gsvc_octree_expand")
    return int(err.item()), out.cpu().numpy()


def _expand_ref(nodes, occ, incl, capacity, size):
    want = np.full(size, -1, np.int64)
    err = 0
    for i, m in enumerate(occ.tolist()):
        if m == 0 or incl[i] > capacity:
            err = 8
            continue
        at = int(incl[i]) - _popcount(m)
        key = 0 if nodes is None else int(nodes[i]) << 3
        for c in range(8):
            if (m >> c) & 1:
                want[at] = key | c
                at += 1
    return err, want


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_popcount_and_expand_equal_a_loop_over_bits(n):
    from gsvc_amd import _lib
    dev = torch.device("cuda")
    occ0 = _masks(n, n, with_zero=True)                        # popcount takes any mask, 0 included
    cnt = torch.full((n + 2,), -1, dtype=torch.int64, device=dev)
    occ_d = torch.from_numpy(occ0).to(dev)
    _lib.check(_lib.lib().gsvc_octree_popcount(_lib.ptr(occ_d), n, _lib.ptr(cnt[1:]), _lib.current_stream(dev)), "gsvc_octree_popcount")
    got = cnt.cpu().numpy()
    assert got[0] == -1 and got[-1] == -1 and got[1:-1].tolist() == [_popcount(m) for m in occ0]
    if n >= 256:
        assert set(occ0.tolist()) == set(range(256))
    occ = _masks(n, n + 1)
    if n >= 255:
        assert set(occ.tolist()) == set(range(1, 256))
    incl = np.cumsum([_popcount(m) for m in occ]).astype(np.int64)
    total = int(incl[-1])
    rng = np.random.default_rng(n)
    parents = np.sort(rng.integers(0, 1 << 45, n)).astype(np.int64)
    for nodes in (None, parents):                              # the root level has no parent keys
        err, out = _expand(nodes, occ, incl, total, total + 9)
        ref_err, want = _expand_ref(nodes, occ, incl, total, total + 9)
        assert err == ref_err == 0 and np.array_equal(out, want) and (out[total:] == -1).all()
    # an empty mask: bit 8; the other nodes' children are where they belong
    if n > 1:
        occ_z = occ.copy()
        occ_z[n // 2] = 0
        err, out = _expand(parents, occ_z, incl, total, total + 9)
        ref_err, want = _expand_ref(parents, occ_z, incl, total, total + 9)
        assert err == ref_err == 8 and np.array_equal(out, want)
    # fewer places than children: bit 8 and nothing at or behind `capacity` (the buffer itself is full-sized)
    cap = total - max(1, total // 3)
    err, out = _expand(parents, occ, incl, cap, total + 9)
    ref_err, want = _expand_ref(parents, occ, incl, cap, total + 9)
    assert err == ref_err == 8 and (out[cap:] == -1).all() and np.array_equal(out, want)


def _demorton_ref(key):
    xyz = [0, 0, 0]
    for b in range(16):
        xyz[0] |= ((key >> (3 * b + 2)) & 1) << b
        xyz[1] |= ((key >> (3 * b + 1)) & 1) << b
        xyz[2] |= ((key >> (3 * b)) & 1) << b
    return xyz


@functools.lru_cache(maxsize=None)
def _keys():
    rng = np.random.default_rng(48)
    keys = [0, (1 << 48) - 1] + [1 << b for b in range(48)] + [int(v) for v in rng.integers(0, 1 << 48, 2000)]
    return np.array(keys, np.int64), np.array([_demorton_ref(k) for k in keys], np.int64)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2050])
def test_demorton_equals_a_loop_over_bits(n):
    from gsvc_amd import _lib
    dev = torch.device("cuda")
    keys, want = _keys()
    assert want[1].tolist() == [65535, 65535, 65535] and want[2 + 2].tolist() == [1, 0, 0] and want[2 + 47].tolist() == [32768, 0, 0]
    keys, want = (keys[-n:], want[-n:]) if n == 1 else (keys[:n], want[:n])
    out = torch.full((3 * n + 6,), -1, dtype=torch.int64, device=dev)
    k_d = torch.from_numpy(np.ascontiguousarray(keys)).to(dev)
    _lib.check(_lib.lib().gsvc_morton_decode(_lib.ptr(k_d), n, _lib.ptr(out[3:]), _lib.current_stream(dev)), "gsvc_morton_decode")
    got = out.cpu().numpy()
    assert (got[:3] == -1).all() and (got[-3:] == -1).all() and np.array_equal(got[3:-3].reshape(n, 3), want)
