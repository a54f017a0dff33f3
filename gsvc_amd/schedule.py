"""How a fitting step is scheduled: whether it is GPU-bound, and the side streams that decision turns on.

One decision per generation pass (``gpu_bound``, recorded on the batch as ``gpu_bound`` / ``small_work``) picks the small-work
stream for the sampled rate and the regularisers, the event under the rasterizer, the weight gradients' stream, the early plan and
the MLP launch forms (``host_bound_step``).  The streams come from one per-device registry, each created once.
"""
from __future__ import annotations

import contextlib
import os
import time

import torch

from . import switches

GPU_BOUND_MIN_ROWS = 150_000       # visible anchor rows of a step from which it counts as GPU-bound: below, the step is host-bound
                                   # (configs[3]: 58 k rows) and the extra events / stream switches only cost host time
# ... unless the Trainer has MEASURED which side bounds its steps (round 5): the row count says nothing about the rasterizer's load, and
# late in a fit a 100 k-anchor model (80 k rows) spends 7 ms per step on the GPU — its Gaussians cover 57 tiles each — while the host
# needs 5.  The host only ever blocks at the step's two waits (the plan's counts, the renders' counters): what it blocks there per step
# is the GPU's lead over it.


class StepContext:
    """The measurement belongs to the Trainer that made it (as module globals two Trainers of one process clobbered
    each other's): ``gpu_bound_hint`` (None = no measurement yet: the row count decides) and the seconds the host spent blocked in the
    step's waits since its Trainer last read them.  A Trainer makes its own context current for the duration of each of its steps
    (``using``); callers without a Trainer (render loops, tests) see the neutral default."""
    __slots__ = ("gpu_bound_hint", "host_blocked_s", "flips")

    def __init__(self):
        self.gpu_bound_hint, self.host_blocked_s, self.flips = None, 0.0, 0


_DEFAULT_CONTEXT = StepContext()
# a plain module global, not a thread-local: the generation's backward, the early-plan hook and the blocked waits run on autograd's
# device thread and must see the step's context
step_context = _DEFAULT_CONTEXT

# few rows: the step's time is the host's -> the MLP layer launches prefer fewer, multi-product launches (gsvc_amd.mlp); written by
# each generation pass (gsvc_amd.generate.generate_neural_gaussians_many) and read by every MLP launch until the next one
host_bound_step = False


@contextlib.contextmanager
def using(ctx):
    """``ctx`` is the current context inside, the previous one again afterwards (also after an error)."""
    global step_context
    prev, step_context = step_context, ctx
    try:
        yield ctx
    finally:
        step_context = prev


def gpu_bound(rows) -> bool:
    """Should this step spend host time (events, stream switches, separate launches) to save GPU time?"""
    # (the measurement only ever ADDS steps to the GPU-bound side: a caller that synchronises every step — float(loss) — never lets the
    # host block in the step's own waits, and must not lose what the row count alone already grants)
    return rows >= GPU_BOUND_MIN_ROWS or bool(step_context.gpu_bound_hint)


def blocked_wait(event):
    """``event.synchronize()``, the time the host spent in it added to the current context (the Trainer's bound detector)."""
    t0 = time.perf_counter()
    event.synchronize()
    step_context.host_blocked_s += time.perf_counter() - t0


# ---- the side streams -------------------------------------------------------------------------------------------------------
_STREAMS = {}


def _streams(key, device, n):
    s = _STREAMS.get(key)
    if s is None:
        s = _STREAMS[key] = [torch.cuda.Stream(device=device) for _ in range(n)]
    return s


def small_work_stream(dev):
    """The small launch-bound pieces that do not read the rasterizer's output (the sampled rate, the regularisers, the optical-flow
    term, the table bits) run on this stream, under the compositing kernels instead of in front of or behind them."""
    return _streams(("small_work", dev.index), dev, 1)[0]


def wgrad_stream(dev):
    """The stream of the generators' / mlp_deform's weight-gradient products in a GPU-bound step's backward (``backward_streams``)."""
    return _streams(("wgrad", dev.index), dev, 1)[0]


def raster_streams(device, renders):
    """Two side streams per device for the independent renders of a step (GSVC_RASTER_STREAMS=1: everything on the current
    stream)."""
    n = switches.RASTER_STREAMS
    if n <= 1 or renders < 2 or torch.device(device).type != "cuda":
        return []
    return _streams(("raster", torch.device(device).index, n), device, n)


def record_on(stream, *objs):
    """``record_stream(stream)`` on every CUDA tensor in ``objs`` (tensors, lists / tuples of them, objects whose attributes hold
    them; None is skipped).  A tensor allocated on the step's stream and READ on the small-work stream must tell the caching
    allocator so: autograd releases saved tensors as soon as a node's backward is enqueued, and a block returned to the step's
    pool while the other stream's kernel is still queued could be handed to — and overwritten by — the next main-stream kernel
    (ADVICE round 4).  The allocator then holds the block back until the work queued on ``stream`` at the time of the free is done."""
    seen = set()

    def walk(o, depth):
        if o is None or id(o) in seen:
            return
        seen.add(id(o))
        if isinstance(o, torch.Tensor):
            if o.is_cuda:
                o.record_stream(stream)
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v, depth)
        elif isinstance(o, dict):
            for v in o.values():
                walk(v, depth)
        elif depth > 0 and hasattr(o, "__dict__") and not isinstance(o, torch.nn.Module):
            for v in vars(o).values():
                walk(v, depth - 1)
    for o in objs:
        walk(o, 1)


# ---- the backward of a GPU-bound step -----------------------------------------------------------------------------------------
_armed = None      # the weight-gradient stream while a backward_streams scope offers it and no chain backward has taken it yet
_depth = 0         # open backward_streams scopes (a backward inside a backward's hook): only the outermost one arms and restores


def take_wgrad_stream():
    """The armed weight-gradient stream, or None: the first chain backward (gsvc_amd.mlp._GenerateAll) inside a ``backward_streams``
    scope takes it and queues its dW products there; any later one in the same scope runs on the step's stream.  A batched step, the
    only one that opens the scope, makes one generation pass and so one chain backward."""
    global _armed
    st, _armed = _armed, None
    return st


@contextlib.contextmanager
def backward_streams(dev, params):
    """Scope of a GPU-bound step's backward: the caller opens it when the batch's ``small_work`` is set (GPU-bound and not
    GSVC_NO_RATE_OVERLAP — so that switch keeps the weight gradients on the step's stream as well).

    * The graph has nodes on the small-work stream: a parameter used on both streams gets its gradient from two — intended (the
      engine orders them), so torch's warning about it is off for THIS backward only.
    * The weight-gradient stream is armed (``take_wgrad_stream``) unless GSVC_NO_WGRAD_OVERLAP is set or one of ``params`` (the
      generators' / mlp_deform's) already has a ``.grad``: the products write the gradients on the side stream and autograd takes them
      on the step's stream, which is race-free only while it steals them into an empty ``.grad``.
    * Leaving it, the current stream waits for the weight-gradient stream (if armed) and for the small-work stream: a parameter only
      the small-work stream touched (the priors' networks, read by the deferred rate alone) has its gradient accumulated THERE, and
      without this wait Adam occasionally read it half written (run-to-run drift of the rate model)."""
    global _armed, _depth
    set_warn = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
    if set_warn is not None:
        set_warn(False)
    _depth += 1
    wgrad = None
    if _depth == 1 and not switches.NO_WGRAD_OVERLAP and all(p.grad is None for p in params):
        wgrad = _armed = wgrad_stream(dev)
    try:
        yield
    finally:
        _depth -= 1
        main = torch.cuda.current_stream(dev)
        if wgrad is not None:
            _armed = None
            main.wait_stream(wgrad)          # the optimizer, the reducer: behind the last product
        main.wait_stream(small_work_stream(dev))
        # torch offers a setter only (no getter to save the caller's choice): a caller who has switched the warning off for the whole
        # process says so once with GSVC_KEEP_STREAM_WARNING_OFF=1 and this scope then leaves it off
        if set_warn is not None and _depth == 0 and not os.environ.get("GSVC_KEEP_STREAM_WARNING_OFF"):
            set_warn(True)
