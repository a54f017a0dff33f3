"""The attribute coder's kernels (gsvc_amd/csrc/ans.hip) held to the independent integer statement of their specification
(oracle/ans_oracle.py) where nothing held them before: the model records of k_ans_model value by value, the bytes of
k_ans_encode / k_ans_scan / k_ans_pack and the symbols of k_ans_decode at the shapes of tests/_ans_cases.py (record groups of 64
segments, the 1024-thread scan, the 16-record prefetch) under extreme models and under models that send almost every symbol
through the decoder's search, gsvc_ans_decode_many's batches of 16 non-empty jobs, and the refusal of damaged streams.
Everything is compared for equality: bytes, integers, error codes."""
import numpy as np
import pytest
import torch

from tests import _ans_cases as K

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _d(a):
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the cases' arrays are read-only)


def _decode_direct(stream: bytes, mu_d, sigma_d):
    """gsvc_ans_decode through the C ABI with a caller-owned, sentinel-filled scratch buffer: (error word, symbols, the scratch as
    uint32 [records, 8])."""
    from gsvc_amd import _lib, codec
    L = _lib.lib()
    dev = mu_d.device
    ps = codec.prepare_streams([stream], dev)[0]
    nbytes = int(L.gsvc_ans_decode_scratch_bytes(ps.n, ps.seg_len))
    scratch = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=dev)
    sym = torch.full((ps.n,), -7777, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(L.gsvc_ans_decode(_lib.ptr(ps.bytes_d), _lib.ptr(ps.offs_d), _lib.ptr(mu_d), _lib.ptr(sigma_d), ps.n, ps.smin, ps.smax,
                                 ps.seg_len, _lib.ptr(sym), _lib.ptr(err), _lib.ptr(scratch), _lib.current_stream(dev)), "gsvc_ans_decode")
    return int(err.item()), sym.cpu().numpy(), scratch.cpu().numpy()[:nbytes - 16].view("<u4").reshape(-1, 8)


@pytest.mark.parametrize("name", K.RECORD_CASES)
def test_model_records_equal_the_specifications_cdf(name):
    """Record of symbol t of segment g at [(g / 64) seg_len + t] 64 + g % 64: (C(s0 - 1), C(s0), C(s0 + 1), C(s0 + 2), bits of mu,
    bits of sigma, 0, 0) with s0 the clamped mode; records of no symbol (the padding of the last group) are not written."""
    from oracle import ans_oracle
    seg_len, smin, smax, sym, mu, sigma = K.case(name)
    code, back, rec = _decode_direct(K.oracle_stream(name), _d(mu), _d(sigma))
    assert code == 0 and np.array_equal(back, sym)
    n = sym.size
    assert rec.shape[0] == (K.n_segments(seg_len, n) + 63) // 64 * 64 * seg_len
    s0 = K.mode_of(mu, smin, smax)
    m64, inv = ans_oracle._model(mu, sigma)
    want = np.full(rec.shape, SENTINEL * 0x01010101, dtype=np.uint32)
    i = np.arange(n)
    g, t = i // seg_len, i % seg_len
    at = ((g >> 6) * seg_len + t) * 64 + (g & 63)
    assert np.unique(at).size == n
    for k in range(n):
        want[at[k], :4] = [ans_oracle.cdf(int(s0[k]) + d, m64[k], inv[k], smin, smax) for d in (-1, 0, 1, 2)]
    want[at, 4], want[at, 5], want[at, 6:] = mu.view(np.uint32), sigma.view(np.uint32), 0
    bad = np.flatnonzero((rec != want).any(axis=1))
    assert bad.size == 0, (bad.size, int(bad[0]), rec[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.parametrize("name", K.BYTE_CASES)
def test_bytes_and_symbols_equal_the_specifications(name):
    from gsvc_amd import codec
    from oracle import ans_oracle
    seg_len, smin, smax, sym, mu, sigma = K.case(name)
    mu_d, sigma_d = _d(mu), _d(sigma)
    want = K.oracle_stream(name)
    got = codec.ans_encode(_d(sym), mu_d, sigma_d, smin, smax, seg_len=seg_len)
    assert got == want, (len(got), len(want), next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None))
    assert np.array_equal(ans_oracle.decode(got, mu, sigma), sym)
    assert np.array_equal(codec.ans_decode(want, mu_d, sigma_d).cpu().numpy(), sym)


# 40 jobs, 35 of them non-empty: batches of 16 + 16 + 3; empty jobs first, inside the first batch, first of the second batch, and the
# last two
_EMPTY = (0, 16, 18, 38, 39)


def _many(streams, models):
    """One gsvc_ans_decode_many call: (per-job error words, per-job symbols)."""
    import ctypes as C
    from gsvc_amd import _lib, codec
    L = _lib.lib()
    dev = torch.device("cuda")
    live = [k for k, st in enumerate(streams) if st is not None]
    prep = dict(zip(live, codec.prepare_streams([streams[k] for k in live], dev)))
    errs = torch.zeros(len(streams), dtype=torch.int32, device=dev)
    arr = (_lib.AnsDecodeJobC * len(streams))()
    keep, out = [], []
    for k, st in enumerate(streams):
        d = arr[k]
        if st is None:
            d.n, d.min_symbol, d.max_symbol, d.seg_len = 0, 0, 1, 1
            out.append(None)
            continue
        ps, (mu, sigma) = prep[k], models[k]
        sym = torch.full((ps.n,), -7777, dtype=torch.int32, device=dev)
        scratch = torch.empty(int(L.gsvc_ans_decode_scratch_bytes(ps.n, ps.seg_len)), dtype=torch.uint8, device=dev)
        mu_d, sigma_d = _d(mu), _d(sigma)
        keep += [mu_d, sigma_d, scratch]
        out.append(sym)
        d.bytes, d.seg_offsets, d.mu, d.sigma = ps.bytes_d.data_ptr(), ps.offs_d.data_ptr(), mu_d.data_ptr(), sigma_d.data_ptr()
        d.n, d.min_symbol, d.max_symbol, d.seg_len = ps.n, ps.smin, ps.smax, ps.seg_len
        d.symbols, d.error_flag, d.scratch = sym.data_ptr(), errs[k:].data_ptr(), scratch.data_ptr()
    _lib.check(L.gsvc_ans_decode_many(arr, len(streams), _lib.current_stream(dev)), "gsvc_ans_decode_many")
    torch.cuda.synchronize()
    return errs.cpu().numpy(), [None if s is None else s.cpu().numpy() for s in out]


def test_decode_many_batches_of_sixteen_with_empty_jobs_and_one_bad_job():
    from oracle import ans_oracle
    names = [n for n in K.BYTE_CASES if not n.endswith("-wide")] + [n for n in K.BYTE_CASES if n.endswith("-wide")]
    names = iter(names + names)
    jobs = [None if k in _EMPTY else next(names) for k in range(40)]
    assert sum(j is not None for j in jobs) == 35
    assert len({(K.case(j)[0], K.case(j)[3].size, K.case(j)[1], K.case(j)[2]) for j in jobs if j}) >= 25      # (seg_len, n, range) differ
    streams = [None if j is None else K.oracle_stream(j) for j in jobs]
    models = [None if j is None else K.case(j)[4:6] for j in jobs]
    errs, syms = _many(streams, models)
    assert not errs.any(), errs
    for j, s in zip(jobs, syms):
        assert (s is None) if j is None else np.array_equal(s, K.case(j)[3]), j
    # a job of the second batch whose last segment is cut below its 4 state bytes: code 3, set before anything of it is read
    bad_job = 25
    st = streams[bad_job]
    n_seg = ans_oracle.HEADER.unpack_from(st, 0)[6]
    sizes = np.frombuffer(st, dtype="<u4", count=n_seg, offset=ans_oracle.HEADER.size).astype(np.int64)
    cut = int(sizes[-1]) - 3
    assert cut >= 1
    sizes[-1] = 3
    streams[bad_job] = st[:ans_oracle.HEADER.size] + sizes.astype("<u4").tobytes() + st[ans_oracle.HEADER.size + 4 * n_seg:len(st) - cut]
    errs, syms = _many(streams, models)
    want = np.zeros(40, np.int32)
    want[bad_job] = 3
    assert np.array_equal(errs, want), errs
    seg_len, _, _, sym = K.case(jobs[bad_job])[:4]
    first_of_last = (n_seg - 1) * seg_len
    for k, (j, s) in enumerate(zip(jobs, syms)):
        if k == bad_job:
            assert np.array_equal(s[:first_of_last], sym[:first_of_last]) and (s[first_of_last:] == -7777).all()
        else:
            assert (s is None) if j is None else np.array_equal(s, K.case(j)[3]), j


def test_every_single_bit_flip_of_a_payload_is_refused_as_the_specification_refuses_it():
    """The 40-symbol stream of tests/test_ans_cases_cpu.py: the strict oracle refuses all 264 single-bit flips of its payload, and
    so must the kernel.  (Without the end-of-segment check — error 6 — flips that change symbols came back with error word 0.)"""
    sym, mu, sigma, stream, at = K.flip_case()
    mu_d, sigma_d = _d(mu), _d(sigma)
    code, back, _ = _decode_direct(stream, mu_d, sigma_d)
    assert code == 0 and np.array_equal(back, sym)
    bits = 8 * (len(stream) - at)
    assert bits == 264
    codes = [_decode_direct(K.flipped(stream, at, b), mu_d, sigma_d)[0] for b in range(bits)]
    print("error words of the 264 flips:", {c: codes.count(c) for c in sorted(set(codes))})
    accepted = [b for b, c in enumerate(codes) if c == 0]
    assert not accepted, (len(accepted), accepted[:8])
    assert set(codes) <= {4, 5, 6}


def test_a_segment_one_byte_too_long_or_too_short_is_refused():
    from oracle import ans_oracle
    sym, mu, sigma, stream, at = K.flip_case()
    mu_d, sigma_d = _d(mu), _d(sigma)
    n_seg = K.n_segments(K.FLIP_SEG_LEN, K.FLIP_N)
    sizes = np.frombuffer(stream, dtype="<u4", count=n_seg, offset=ans_oracle.HEADER.size)
    assert (sizes >= 5).all()
    from gsvc_amd import _lib, codec
    with pytest.raises(_lib.GsvcError, match="code 6"):
        codec.ans_decode(K.resized_segment(stream, 2, +1), mu_d, sigma_d)
    for seg in range(n_seg):
        assert _decode_direct(K.resized_segment(stream, seg, +1), mu_d, sigma_d)[0] == 6, seg      # a byte nobody reads
        assert _decode_direct(K.resized_segment(stream, seg, -1), mu_d, sigma_d)[0] == 5, seg      # the last byte is missing
