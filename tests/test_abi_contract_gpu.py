"""The contract every entry point of include/gsvc_hip.h states — nothing is allocated, freed or synchronised inside a call, and every
launch, helper kernel and memset goes to the `stream` it is given, so every call may be captured into a hipGraph — held for every
entry family, one small case each (tests/_abi_contract_cases.py; tests/test_abi.py counts that no entry point is left out).  The
values are the business of each family's own float64 / bit-exact test; here a case is run five ways and its buffers compared as
bits, every word of every allocation, the tail pads included:

  1. warm-up     the case's calls once, eagerly, on the default stream (this is also how they are recorded).  A process's first call
                 through an entry family may set function attributes or upload a table: include/gsvc_hip.h asks for one eager
                 call per family before a capture.  Every return code is 0.
  2. side stream the inputs put back, the same calls on a fresh side stream, that stream alone synchronised: `eager`.  Again: the
                 same bits (the library runs in its deterministic mode for this module).  Where a family's sums are float atomics
                 in an order that mode does not fix (q_rows, training_statis), the buffers that differ are held, here and after
                 each replay, to the family's own float64 rule, which the case brings along from the family's test module; every
                 other buffer of the case is still compared as bits.
  3. capture     every word the calls write pre-filled with the NaN-payload sentinel, the calls captured on the side stream.  Every
                 return code is 0, the capture ends without an error (a synchronisation or an allocation would have failed it), and
                 every buffer still holds what it held: a launch or a memset that escaped to another stream would have run.
  4. replay      the inputs put back, one replay: `eager`, bit for bit.
  5. new data    a second data set from the same builders copied over the inputs in place; its expected bits come from an eager run
                 in buffers of its own.  One more replay gives exactly those: nothing the host derived from the first data set, or
                 read back from the device, was baked into the graph.

Every graph is a linear chain on one stream (no case hands an entry a second stream; the forked weight-gradient form keeps
tests/test_mlp_gpu.py::test_weight_gradients_on_their_own_stream_are_the_same_gradients) and is replayed twice, one replay after the
other.
"""
import os
import subprocess
import sys

import pytest
import torch

from tests import _abi_contract_cases as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def deterministic_mode():
    """gsvc_set_deterministic(1): the float-atomic scatters add in a fixed order.  The switch is put back afterwards."""
    from gsvc_amd import _lib
    was = _lib._deterministic
    _lib.lib().gsvc_set_deterministic(1)
    yield
    _lib.lib().gsvc_set_deterministic(int(was))


def _on(side, rec):
    """rec's calls on `side`, that stream alone synchronised; the bits of every buffer afterwards."""
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        rcs = rec.run(side)
    side.synchronize()
    assert rcs and not any(rcs), rcs
    return [b.clone() for b in rec.buffers]


def _differing(got, want, only=None):
    """[(buffer, differing bytes, bytes, first differing byte, what it holds, what it should hold)] over the buffers `only` names."""
    out = []
    for k, (g, w) in enumerate(zip(got, want)):
        if (only is None or k in only) and not torch.equal(g, w):
            at = int((g != w).nonzero()[0])
            lo = at // 4 * 4
            out.append((k, int((g != w).sum()), g.numel(), at, bytes(g[lo:lo + 4].tolist())[::-1].hex(), bytes(w[lo:lo + 4].tolist())[::-1].hex()))
    return out


@pytest.mark.parametrize("case", A.CASES, ids=[c.name for c in A.CASES])
def test_calls_go_to_their_stream_and_replay_from_a_graph(case):
    # 1. warm-up (and recording)
    rec = A.Recording(case.script)
    assert rec.calls and not any(rec.eager_rc), (rec.eager_rc, [c[0] for c in rec.calls])
    assert rec.names() == set(case.entries) | set(case.also), sorted(rec.names() ^ (set(case.entries) | set(case.also)))
    assert any(bool(w.any()) for w in rec.written)
    # 2. eager on a side stream, twice
    side = torch.cuda.Stream()
    eager = _on(side, rec)
    rec.restore()
    again = _on(side, rec)
    loose, exact = rec.loose, set(range(len(eager))) - rec.loose
    assert not _differing(again, eager, exact), ("two eager runs differ", _differing(again, eager, exact))
    if loose:
        rec.check()
    # 3. capture: nothing runs, nothing leaves the stream
    rec.restore(sentinel_outputs=True)
    before = rec.before_replay()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rcs = rec.run(side)
    torch.cuda.synchronize()
    assert rcs and not any(rcs), rcs
    assert not _differing(rec.bits(), before), ("something ran during the capture", _differing(rec.bits(), before))
    # 4. one replay
    rec.restore()
    g.replay()
    assert not _differing(rec.bits(), eager, exact), ("the replay differs from the eager run", _differing(rec.bits(), eager, exact))
    if loose:
        rec.check()
    # 5. a replay on new contents
    other = A.Recording(case.script, seed=1)
    assert not any(other.eager_rc)
    rec.refill(other)
    want = _on(side, other)
    g.replay()
    got = rec.bits()
    assert not _differing(got, want, exact), ("the replay on new contents differs from the eager run on them", _differing(got, want, exact))
    if loose:
        rec.check()


_FIRST_ANS_CALL_IN_A_CAPTURE = r"""
import ctypes as C
import torch
from gsvc_amd import _lib
L = _lib.lib()
n, seg_len = 64, 16
sym = torch.zeros(n, dtype=torch.int32, device="cuda")
mu, sigma = torch.zeros(n, device="cuda"), torch.ones(n, device="cuda")
n_seg, cap = int(L.gsvc_ans_segments(n, seg_len)), int(L.gsvc_ans_scratch_bytes(n, seg_len))
scratch, out = torch.zeros(cap, dtype=torch.uint8, device="cuda"), torch.zeros(cap, dtype=torch.uint8, device="cuda")
seg_bytes, seg_offsets = torch.zeros(n_seg, dtype=torch.int32, device="cuda"), torch.zeros(n_seg + 1, dtype=torch.int64, device="cuda")
err, ticks = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, device="cuda")
side = torch.cuda.Stream()


def capture():
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            ticks.add_(1.0)
            rc = L.gsvc_ans_encode(_lib.ptr(sym), _lib.ptr(mu), _lib.ptr(sigma), n, -4, 4, seg_len, _lib.ptr(scratch), _lib.ptr(seg_bytes),
                                   _lib.ptr(seg_offsets), _lib.ptr(out), _lib.ptr(err), C.c_void_p(side.cuda_stream))
    torch.cuda.synchronize()
    return g, rc


g, rc = capture()                      # the process's first coder call, inside a capture: refused, the capture survives
print("FIRST", rc, L.gsvc_last_error().decode())
g.replay()
torch.cuda.synchronize()
print("AFTER_REFUSAL", int(ticks.item()), int(seg_offsets[-1].item()))
L.gsvc_ans_table_checksum()            # the documented first call
g, rc = capture()
print("SECOND", rc)
g.replay()
torch.cuda.synchronize()
print("AFTER_CAPTURE", int(ticks.item()), int(err.item()), int(seg_offsets[-1].item()) > 0)
"""


def test_the_first_coder_call_of_a_process_is_refused_inside_a_capture():
    """The entropy coder's Phi table is uploaded by a synchronous copy on the first use in a process, which a capturing stream must
    not see.  include/gsvc_hip.h makes gsvc_ans_table_checksum() the call to make first; until the table is up, gsvc_ans_encode / _decode /
    _decode_many on a capturing stream return GSVC_E_UNSUPPORTED before doing anything, and the capture goes on.  After the
    checksum call the same capture records the encoder and replays it.  (A fresh process: the table is per process.)"""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-c", _FIRST_ANS_CALL_IN_A_CAPTURE], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = dict(l.split(" ", 1) for l in p.stdout.splitlines() if l.split(" ", 1)[0] in ("FIRST", "AFTER_REFUSAL", "SECOND", "AFTER_CAPTURE"))
    assert lines["FIRST"].startswith("-3 ") and "gsvc_ans_table_checksum() once before the capture" in lines["FIRST"], lines
    assert lines["AFTER_REFUSAL"] == "1 0", lines          # the rest of the capture replays; the encoder was not in it
    assert lines["SECOND"] == "0" and lines["AFTER_CAPTURE"] == "2 0 True", lines
