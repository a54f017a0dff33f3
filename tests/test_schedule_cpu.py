"""The step's scheduling context (gsvc_amd/schedule.py): a Trainer's measured bound and blocked time are current for the duration of
its steps only — the repeat after an overflow included, an error included — and two Trainers that alternate steps each read and add
to their own.  CPU Trainers with the step body replaced: what is checked is the context around it, not the step."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


class _Event:
    """Stands for a CUDA event: the host "blocks" ``seconds`` in its synchronize()."""

    def __init__(self, seconds):
        self.seconds = seconds

    def synchronize(self):
        import time
        time.sleep(self.seconds)


def _trainer(monkeypatch, blocked, log, overflow_first=False):
    from tests.test_densify_cpu import _model
    from gsvc_amd import schedule
    from gsvc_amd.arguments import ModelParams, OptimizationParams, PipelineParams
    from gsvc_amd.train import Trainer
    pc = _model(np.load(os.path.join(HERE, "golden", "densify.npz")))
    tr = Trainer(pc, SimpleNamespace(len_z_frames=8), OptimizationParams(), PipelineParams(), ModelParams(), prefetch=False)
    attempts = []

    def body(iteration, frame_idx=None, early=True):
        attempts.append(iteration)
        ctx = schedule.step_context
        log.append((tr, ctx, schedule.gpu_bound(0)))
        schedule.blocked_wait(_Event(blocked))
        if overflow_first and len(attempts) == 1:
            return None          # an instance buffer overflowed: Trainer.step repeats the step
        return SimpleNamespace(loss=torch.zeros(()))
    monkeypatch.setattr(tr, "_step", body)
    return tr


def test_a_trainers_context_is_current_inside_its_steps_only(monkeypatch):
    monkeypatch.delenv("GSVC_DETERMINISTIC", raising=False)
    monkeypatch.delenv("GSVC_NO_ADAPTIVE_BOUND", raising=False)
    from gsvc_amd import schedule
    default = schedule.step_context
    log = []
    a = _trainer(monkeypatch, 0.02, log, overflow_first=True)
    b = _trainer(monkeypatch, 0.0, log)
    assert a._ctx is not default and b._ctx is not default and a._ctx is not b._ctx
    a._ctx.gpu_bound_hint, b._ctx.gpu_bound_hint = True, False       # (the first steps do not measure: _update_bound keeps these)
    for it in range(1, 4):
        for tr in (a, b):
            before = len(log)
            tr.step(it, frame_idx=2)
            assert schedule.step_context is default
            steps = log[before:]
            # every attempt of the step (A's first step is repeated) ran in this trainer's context and read its hint
            assert steps and all(t is tr and ctx is tr._ctx and bound is bool(tr._ctx.gpu_bound_hint) for t, ctx, bound in steps)
            assert len(steps) == (2 if (tr is a and it == 1) else 1)
        # what each trainer blocked in its last step is its own (A: 20 ms per attempt; B: nothing)
        assert a._ctx.host_blocked_s >= 0.02 and b._ctx.host_blocked_s < 0.01
    # outside a step: the neutral default, and a wait there adds to nobody's measurement
    assert schedule.gpu_bound(0) is False
    blocked_a, blocked_b = a._ctx.host_blocked_s, b._ctx.host_blocked_s
    schedule.blocked_wait(_Event(0.01))
    assert (a._ctx.host_blocked_s, b._ctx.host_blocked_s) == (blocked_a, blocked_b)
    a.close()
    b.close()


def test_a_fresh_trainer_has_its_state_declared(monkeypatch):
    """What tools and the benchmark read of a Trainer exists from its constructor on, and a removed argument is an error."""
    from gsvc_amd.arguments import ModelParams, OptimizationParams, PipelineParams
    from gsvc_amd.train import Trainer
    tr = _trainer(monkeypatch, 0.0, [])
    assert tr.repeated_steps == 0 and tr.early_steps == 0 and tr.bound_log == [] and tr._last_idx is None
    with pytest.raises(TypeError):
        Trainer(tr.pc, tr.dataset, OptimizationParams(), PipelineParams(), ModelParams(), prefetch=False, shard_optimizer=True)
    tr.close()


def test_a_failing_step_restores_the_previous_context(monkeypatch):
    from gsvc_amd import schedule
    default = schedule.step_context
    tr = _trainer(monkeypatch, 0.0, [])

    def fail(*a, **k):
        assert schedule.step_context is tr._ctx
        raise RuntimeError("step failed")
    monkeypatch.setattr(tr, "_step", fail)
    with pytest.raises(RuntimeError, match="step failed"):
        tr.step(1, frame_idx=2)
    assert schedule.step_context is default
    tr.close()
