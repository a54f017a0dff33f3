"""The fitting step: 4 renders (2 adjacent frames x 2 opposite views), distortion + regularisers + optical-flow
consistency + lambda * rate, backward, densification statistics, Adam.

Same loss and order of operations as the step body of reference pipeline/train.py:325-462,559-581; logging,
evaluation, tensorboard and the codec calls around it are out of scope.  Differences in mechanism: no per-step
`.item()` / synchronize (the reference syncs ~10x per step for logging), the hash-table bit count stays on the
device, and under torch.distributed each rank steps on its own frame pair and gradients are averaged with one
collective (gsvc_amd/dist.py).  Anchor growing/pruning runs at the reference's cadence (gsvc_amd/densify.py).
"""
from __future__ import annotations

import os
import random
from dataclasses import dataclass

import contextlib

import torch

from . import dist as gdist
from . import schedule, switches
from .generate import GenerateMode, region
from .loss_utils import StepDistortion, calc_optical_loss, render_regs
from .optim import FusedAdam
from .ortho_gaussian_renderer import plan_views, render, render_many
from .rasterizer import resolve_deferred
from .train_util import TrainingController


@dataclass
class StepOutput:
    """What a step hands back — all of it graph-free: the loss and images are detached, and so are the tensors inside ``renders``
    (their backward has run; ``_release_graph``).  Differentiate through ``render()`` / ``render_many()`` directly instead."""
    loss: torch.Tensor
    image1: torch.Tensor
    image2: torch.Tensor
    renders: tuple
    active_gaussians: torch.Tensor  # sum over the 4 renders of Gaussians with radius > 0 (device scalar)
    frame_idx: int


@dataclass
class _Step:
    """One attempt of a step: what its stages (``Trainer._step_body``) hand to one another; each stage's docstring names the fields it
    reads and sets.  It holds the attempt's autograd graph (terms, loss), so it lives in ``_step_body``'s frame only: not on the
    Trainer, not in the StepOutput, not in a hook's closure."""
    iteration: int
    frame_idx: int
    early: bool                         # this attempt may run the early tail (the repeat after an overflow may not)
    mode: object                        # the phase's GenerateMode
    zown: object = None                 # the z-range ownership in force, or None
    plan: object = None                 # the StepPlan queued for this frame pair, when it still matches
    frame1: object = None
    frame2: object = None
    renders: tuple = None               # (frame 1 front, back, frame 2 front, back)
    batch: object = None                # the renders' StepBatch; None in the unbatched step
    ovf_handle: object = None           # the replicas' overflow reduction in flight (batched step)
    image1: torch.Tensor = None         # the two-view frames
    image2: torch.Tensor = None
    terms: list = None                  # the loss's scalar terms, the image terms first
    weights: list = None                # their weights, as host values
    const: float = 0.0
    loss: torch.Tensor = None


def _release_graph(renders):
    """The step's backward has run: what the caller keeps of the step (the renders, their generated Gaussians, the batch) must not
    keep the autograd graph alive.  A caller that holds the previous step's output while the next step runs — every training loop
    does: ``out = trainer.step(i)`` — otherwise keeps that graph's AccumulateGrad nodes, the engine reuses them with the streams
    they were created on, and the extra waits it then inserts undo the overlap of the small-work stream (measured: 6.6 -> 7.1 ms)."""
    T = torch.Tensor
    seen = set()

    def strip(obj):
        d = getattr(obj, "__dict__", None)
        if d is None or id(obj) in seen:
            return
        seen.add(id(obj))
        for k, v in d.items():
            if type(v) is T and v.grad_fn is not None:
                d[k] = v.detach()
    for r in renders:
        strip(r)
        g = r.generated_gaussians
        if g is not None:
            strip(g)
            strip(g.batch)


def hash_grid_bits(pc):
    """Bernoulli code length of the binarised hash tables (reference pipeline/train.py:456:
    ``get_binary_vxl_size((get_encoding_params() + 1) / 2)``).  The count of ones is taken table by table from the binarised
    tables the grid lookups already made ({-1, +1}: ones = (sum + n) / 2) instead of from a 14 MB concatenation of them."""
    tables = grid_tables(pc)
    if not (pc.ste_binary and all(hasattr(g, "embeddings") for g in tables)):
        return get_binary_vxl_size_device((pc.get_encoding_params() + 1) / 2)
    from .encodings import CountBits, binarized_tables
    embs = binarized_tables(tables)
    cache0 = getattr(tables[0], "step_cache", None) or {}
    if "counts_all" in cache0 and cache0["counts_all"][1] == tuple(id(g) for g in tables):
        # every table was binarised by one launch that also counted its +1 entries: the term and its gradient are written
        # on that count vector (two one-thread launches; the tables receive it inside their straight-through backward)
        return CountBits.apply(cache0["counts_all"][0], sum(e.numel() for e in embs))
    counts = [(getattr(g, "step_cache", None) or {}).get("ones") for g in tables]
    return _TableBits.apply(torch.cat(counts) if all(c is not None for c in counts) else None, *embs)


class _TableBits(torch.autograd.Function):
    """bits = n1 (-log2 p) + n0 (-log2 (1 - p)) + 32 over the {-1, +1} tables, p = n1 / n clamped to [1e-6, 1 - 1e-6]
    (reference utils/encodings.py:34-51).  d bits / d n1 = log2((1 - p) / p) — the terms through p cancel exactly where p is not
    clamped and vanish where it is — and n1 = (sum of the entries + n) / 2, so every table entry receives the same number:
    the backward is one scalar expression and an expand instead of a dozen one-element kernels each way."""

    @staticmethod
    def forward(ctx, counts, *tables):
        total = sum(t.numel() for t in tables)
        # counts: the +1 entries of every table, counted by the kernel that binarised it (else: from the tables' sums)
        ones = counts.sum() if counts is not None else (torch.stack([t.sum() for t in tables]).sum() + total) / 2
        p = torch.clamp(ones / total, min=1e-6, max=1 - 1e-6)
        ctx.save_for_backward(p)
        ctx.shapes = [t.shape for t in tables]
        return ones * (-torch.log2(p)) + (total - ones) * (-torch.log2(1 - p)) + 32

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        coef = g * 0.5 * torch.log2((1 - p) / p)
        return (None,) + tuple(coef.expand(sh) for sh in ctx.shapes)


def grid_tables(pc):
    enc = pc.encoding_xyz
    return [enc.encoding_xyz, enc.encoding_xy, enc.encoding_xz, enc.encoding_yz] if pc.use_2D else [enc]


def get_binary_vxl_size_device(binary_vxl):
    total = binary_vxl.numel()
    ones = binary_vxl.sum()
    p = torch.clamp(ones / total, min=1e-6, max=1 - 1e-6)
    return ones * (-torch.log2(p)) + (total - ones) * (-torch.log2(1 - p)) + 32


def _mean_over_selected(values, r):
    """Mean over the Gaussians a render generated (opacity > 0): all rows of a compacted result, the rows marked
    by ``selection_mask`` of an un-compacted one."""
    if not r.dense:
        return values.mean()
    w = r.selection_mask.to(values.dtype)
    return (values * w).sum() / w.sum()


class Trainer:
    def __init__(self, gaussians, dataset, opt, pipe, model_params, seed: int = 0, batched: bool = True, prefetch: bool = True,
                 weight_maps=None, weight_cell=None):
        # what the step's image terms are and where they are taken: refuses a loss domain or a structural term this dataset cannot have.
        # weight_maps [T, Hc, Wc] (gsvc_amd/wdist.py) weight them per cell; they live on the model's device, each frame of a step takes
        # its own
        if weight_maps is not None and torch.is_tensor(weight_maps):
            weight_maps = weight_maps.to(gaussians._anchor.device)
        self._distortion = StepDistortion(opt, dataset, weight_maps=weight_maps, weight_cell=weight_cell)
        self.weight_maps, self.weight_cell = self._distortion.weight_maps, self._distortion.weight_cell
        self.weighting = None                  # what a log says of the maps (fit_setup.new_fit sets it)
        self.loss_domain, self.loss_matrix, self.distortion = self._distortion.domain, self._distortion.matrix, self._distortion.name
        self.batched = batched
        # prefetch: the next step's frame pair is drawn, its visibility test run and every data-dependent index list of its
        # generation pass queued at the END of a step (gsvc_amd.generate.StepPlan): the next step then starts with one wait
        # for nine counts instead of six device round trips with an idle GPU
        self.prefetch = prefetch and batched and not switches.NO_PREFETCH      # env: A/B timing only
        self._plan = self._plan_idx = self._plan_mode = None
        self.pc, self.dataset, self.opt, self.pipe, self.mp = gaussians, dataset, opt, pipe, model_params
        if gaussians._anchor.is_cuda:
            from .hostbind import bind_to_device
            bind_to_device(gaussians._anchor.device)      # the step is host-bound at small sizes: stay on the GPU's NUMA node
        self.controller = TrainingController(opt)
        self.controller.step()  # iterations are 1-based
        self.rng = random.Random(seed + gdist.rank())
        self.lo, self.hi = gdist.frame_shard(dataset.len_z_frames)
        bg = [1, 1, 1] if model_params.white_background else [0, 0, 0]
        self.background = torch.tensor(bg, dtype=torch.float32)  # host tensor: the kernels take bg by value
        # anchors are trained with learning rate 0 in GSVC (position_lr_init = position_lr_final = 0): their gradient
        # changes nothing, so the batched step does not compute it unless a non-zero rate is configured
        self.anchor_grad = bool(getattr(opt, "position_lr_init", 0.0) or getattr(opt, "position_lr_final", 0.0))
        gaussians.anchor_static = not self.anchor_grad      # the quantised anchors may be cached between steps (prefilter_geometry)
        self.reducer = gdist.GradReducer()
        gdist.plan_group()      # created HERE, where every rank stands at the same point (creating a group is itself collective)
        # GSVC_DP_ZOWN=1: the per-anchor tensors are OWNED by z-range (gsvc_amd.dist.ZRangeOwnership) — gradients of the halo rows go
        # to their owners, updated rows come back — instead of being summed on every replica
        self._zown = None
        if gdist.zrange_enabled() and not (batched and not self.anchor_grad):
            import sys
            sys.stderr.write("gsvc_amd.train: GSVC_DP_ZOWN=1 ignored (needs the batched step and anchors with learning rate 0: an anchor that moves "
                             "could change its owner): replicated exchange\n")
        if gdist.zrange_enabled() and batched and not self.anchor_grad:
            self._zown = gdist.ZRangeOwnership(dataset.len_z_frames, dataset.scale, model_params.threshold)
            assert abs(dataset[self.lo].z - (self.lo - dataset.len_z_frames / 2) / dataset.scale) < 1e-6, "frame z convention"
        gaussians._zown = self._zown      # gsvc_amd.generate._param_means reads the owners' means from it
        self._mask_reg_weight = 0.0
        self._ovf_handle = None
        self._last_idx = None                  # the frame pair of the last attempted step (its repeat after an overflow takes it again)
        self._early = None                     # (params, idx, mode, plan) of an early tail that ran inside this step's backward
        self.repeated_steps = 0                # steps run twice because a rasterizer instance buffer overflowed
        self.early_steps = 0                   # steps whose _scaling / _mask update and next plan ran from inside the backward
        self._w_key = self._w = None           # the loss weights on the device, and the host values they were made from
        self._logged_exchange = None           # which per-anchor gradient exchange the one-time log line last named
        # which side bounds the steps, measured (gsvc_amd.schedule.StepContext.gpu_bound_hint): the host's blocked time per step, smoothed
        self._blocked_ema = None
        self._steps_seen = self._ema_n = 0     # steps, and steps that entered the average
        self.bound_log = []                    # (step, gpu_bound, blocked ms) of the last 32 changes of the decision
        self._ctx = schedule.StepContext()      # this trainer's own measurement (made current for the duration of each of its steps)
        # the generators' and mlp_deform's parameters: the networks whose weight gradients may take a stream of their own
        self._chain_params = [p for m in (gaussians.get_opacity_mlp, gaussians.get_color_mlp, gaussians.get_cov_mlp, gaussians.get_deform_mlp)
                              for p in m.parameters()]

    def close(self):
        """Give the calling thread its CPU affinity back (``__init__`` narrowed it to the GPU's NUMA node: gsvc_amd/hostbind.py;
        GSVC_NO_CPU_BIND=1 never narrows it)."""
        if self.pc._anchor.is_cuda:
            from .hostbind import unbind
            unbind(self.pc._anchor.device)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _two_views(self, frame, mode, retain_grad):
        f = render(frame, self.pc, self.pipe, self.background, retain_grad=retain_grad, mode=mode)
        frame.view_matrix, frame.view_matrix_s = frame.view_matrix_s, frame.view_matrix
        b = render(frame, self.pc, self.pipe, self.background, retain_grad=retain_grad, mode=mode)
        image = (f.rendered_image + torch.flip(b.rendered_image, dims=(-1,))) / 2
        return f, b, image

    def _update_bound(self):
        """The host blocks only at the step's two waits, and what it blocks there is how far the GPU is behind it: over ~0.4 ms per
        step the GPU bounds the step and host-side work that shortens the GPU's (the small-work stream, the early plan, separate
        layer launches) pays; under ~0.1 ms the host does and it does not.  In between the last decision stands (the measures
        themselves move the balance).  The first steps (allocator growth, first launches) are not counted."""
        ctx = self._ctx
        b = ctx.host_blocked_s
        ctx.host_blocked_s = 0.0
        self._steps_seen += 1
        if switches.NO_ADAPTIVE_BOUND or switches.DETERMINISTIC:
            # (deterministic mode: a wall-clock measurement must not pick between the separate and the multi-product layer launches —
            # they round differently — so the row count alone decides, the same way in every run)
            ctx.gpu_bound_hint = None
            return
        if self._steps_seen <= 8:
            return
        self._blocked_ema = b if self._blocked_ema is None else 0.8 * self._blocked_ema + 0.2 * b
        self._ema_n += 1
        if self._steps_seen < 16 or self._ema_n < 8:
            # (the average needs a few steps of its own: a fit that leaves the deterministic mode, or follows a synchronisation, starts
            # it with ONE step's wait — bench.py's first timed steps after its frozen pretrain were decided by a 0.008 ms sample and ran
            # host-bound for 57 steps; until then the row count decides)
            return
        before = ctx.gpu_bound_hint
        if self._blocked_ema > 4e-4:
            ctx.gpu_bound_hint = True
        elif self._blocked_ema < 1e-4:
            ctx.gpu_bound_hint = False
        if ctx.gpu_bound_hint != before:
            # a wall-clock measurement changes which launches the step takes from here on: on record, so that runs can be compared
            ctx.flips += 1
            self.bound_log = self.bound_log[-31:] + [(self._steps_seen, bool(ctx.gpu_bound_hint), 1e3 * self._blocked_ema)]

    def step(self, iteration: int, frame_idx: int | None = None) -> StepOutput:
        # whatever this step's generation, waits and backward read and add to is this trainer's; outside a step, the default context
        with schedule.using(self._ctx):
            self._update_bound()
            if frame_idx is None and self._plan_idx is not None:
                frame_idx = self._plan_idx              # drawn (from the same generator, in the same order) at the end of the last step
            self._early = None
            out = self._step(iteration, frame_idx)
            if out is None:      # a rasterizer instance buffer overflowed (capacity now raised): repeat the step
                self.repeated_steps += 1
                dropped = None
                if self._early is not None:
                    # the guarded early update saw the overflow word and wrote nothing: only its step counts moved.  The plan it
                    # queued is for the NEXT frame pair; the repeat draws its own lists.
                    self.pc.optimizer.rewind(self._early[0])
                    dropped = self._early[3]          # its count exchange is in flight: the tensors stay alive until the repeat is done
                    self._early = None
                elif self.prefetch and self.pc._anchor.is_cuda and gdist.active():
                    # Whether the early tail ran is a rank-LOCAL fact (its row threshold and reducer.complete() depend on the rank's
                    # own views), and it queued a plan = one collective on the plan group.  A rank that did not run it answers with a
                    # matching no-op exchange, so that every rank has issued exactly ONE plan-group collective per attempted step:
                    # otherwise the repeat's end-of-step plan on this rank would pair with the other rank's dropped one and every
                    # later distinct_cap would be one step out of phase between the ranks.
                    dropped = gdist.plan_group_noop(self.pc._anchor.device)
                # the repeat draws its own index lists on EVERY rank (no plan -> dense gradient exchange everywhere): a rank that kept
                # its plan would exchange rows while a rank that dropped its early plan all-reduces
                self._plan = None
                self.pc.optimizer.zero_grad(set_to_none=True)
                out = self._step(iteration, frame_idx if frame_idx is not None else self._last_idx, early=False)     # the same frame pair again
                if out is None:
                    raise RuntimeError("rasterizer instance buffer overflowed twice in a row")
                if dropped is not None and getattr(dropped, "_gmax_work", None) is not None:
                    dropped._gmax_work.wait()
                del dropped
            self.controller.step()
            if self._early is not None:          # the next step's plan was queued from inside the backward (_early_tail)
                _, self._plan_idx, self._plan_mode, self._plan = self._early
                self._early = None
                return out
            self._plan = self._plan_idx = None
            if self.prefetch and self.pc._anchor.is_cuda:
                with torch.no_grad(), region('step.plan'):
                    self._plan_idx = self.rng.randint(self.lo, max(self.lo, self.hi - 1))
                    self._prefetch_frames(self._plan_idx)
                    self._plan_mode = self.controller.render_mode
                    self._plan = plan_views(self._views(self._plan_idx), self.pc, self.pipe, self.background, self._plan_mode)
            return out

    def sync_replicas(self, moments: bool = True):
        """Under z-range ownership (GSVC_DP_ZOWN=1) a replica is only fresh inside its own block + halo: call this (on every rank)
        before anything reads the whole model — evaluation, estimate_final_bits, stream encoding, a checkpoint."""
        if self._zown is not None:
            self._zown.sync_full(self.pc, moments=moments)
        self.pc._zown = None      # outside a step the whole-tensor means are the model's own again (gsvc_amd.generate._param_means)

    def _zown_names(self, mode):
        # TRAININ_STE_ENTROPY renders from detached attributes: only _mask receives a gradient (and only it moves)
        return ("_mask",) if mode == GenerateMode.TRAININ_STE_ENTROPY else gdist.PER_ANCHOR

    def _prefetch_frames(self, idx):
        """A dataset that keeps its pictures in host memory (gsvc_amd.frame.HostResidentCube) starts uploading the next step's pair
        now, on its copy stream (reference pipeline/train.py:407-408 uploads them inside the step)."""
        pf = getattr(self.dataset, "prefetch", None)
        if pf is not None:
            pf(idx)

    def _add_mask_reg(self):
        """Sparse data-parallel exchange: the mask regulariser 5e-4 * mean(sigmoid(_mask)) touches EVERY row of ``_mask`` with the
        same number on every rank (the parameters are replicas), so it stays out of the exchanged gradient — its loss term is taken
        of a detached copy — and its gradient, a closed form, is added on every rank after the exchange."""
        if self._mask_reg_weight:
            pc = self.pc
            with torch.no_grad():
                sg = torch.sigmoid(pc._mask)
                reg = sg * (1.0 - sg) * (self._mask_reg_weight / pc._mask.numel())
                if pc._mask.grad is None:
                    pc._mask.grad = reg
                else:
                    pc._mask.grad.add_(reg)
            self._mask_reg_weight = 0.0

    def _early_tail(self, renders, params):
        """Called from inside the backward, the moment the gradients of ``params`` — ``_scaling`` and ``_mask``, those of the two
        that this phase's step gives a gradient — are complete (the last
        contribution is the late row gather's backward: gsvc_amd.generate._gather_rows): these two tensors are all the next
        step's visibility test and rate sample read that this step changes, so they are updated NOW and the next step's plan
        is queued behind them — its counts reach the host ~2 ms before the GPU finishes this step, and the host, which runs
        ahead of the GPU, never has to let the queue drain at a step boundary.  (With the plan queued behind the optimizer the
        host waited ~1.4 ms per step for it and the GPU then idled until the next step's first kernels arrived.)
        The update is guarded by the rasterizer's overflow words: a step that must be repeated changes nothing."""
        from .train_util import render_mode_at
        pc = self.pc
        with torch.no_grad():
            guards = [r.raster_state.binning[4:8].view(torch.int32) for r in renders]
            if gdist.active():
                # data parallel: the two gradients are final once their collectives (launched by the reducer's hooks, which run
                # before this one) have completed; a step in which they have not gone out yet (no agreed order in the very first
                # one) takes the ordinary end-of-step path.  "Some rank overflowed" guards the update as well.
                if not self.reducer.complete(params):
                    return
                self._add_mask_reg()
                guards = [self._ovf_handle[2]]        # the MAX over the ranks of the four local words (this rank's included)
            pc.optimizer.step(only=params, guards=guards)
            self.early_steps += 1
            idx = self.rng.randint(self.lo, max(self.lo, self.hi - 1))
            self._prefetch_frames(idx)
            mode = render_mode_at(self.controller.current_iteration + 1, self.opt)
            plan = plan_views(self._views(idx), pc, self.pipe, self.background, mode) if mode is not None else None
            self._early = (params, idx, mode, plan)

    def _sparse_dp(self, plan):
        """Row-sparse gradient exchange of the per-anchor tensors: needs the step plan (the rank's distinct visible anchors and the
        largest such count over the ranks) and the replicated Adam; GSVC_DP_SPARSE=0 keeps the dense all-reduce."""
        if not (plan is not None and gdist.active() and self.reducer.enabled and not self.anchor_grad and self._zown is None
                and getattr(plan, "distinct_cap", None) is not None and switches.DP_SPARSE != "0"):
            return False
        # every rank receives the other ranks' row lists (all-gather, padded to the largest): worth it while those rows are fewer
        # than what a ring all-reduce of the dense tensors moves (2 (W - 1) / W of the anchors) — two ranks always, eight ranks
        # only when a rank sees less than a quarter of the anchors.  The same decision on every rank (cap is their maximum).
        return switches.DP_SPARSE == "1" or gdist.sparse_rows_pay(gdist.world_size(), int(self.pc._anchor.shape[0]),
                                                                                  plan.distinct_cap)

    def _views(self, frame_idx):
        """The step's four views: (frame, frame seen from the opposite side) of the two adjacent frames."""
        import copy
        views = []
        for fr in (self._distortion.frame(self.dataset, frame_idx), self._distortion.frame(self.dataset, frame_idx + 1)):
            back = copy.copy(fr)
            back.view_matrix, back.view_matrix_s = fr.view_matrix_s, fr.view_matrix
            views += [fr, back]
        return views

    def _adjust_anchor(self, iteration):
        """Densify / prune (reference pipeline/train.py:567-569).  Under data parallelism every rank must take the same
        decisions: the statistics are summed over ranks first and the random thinning uses a per-iteration seed."""
        opt = self.opt
        if self._zown is not None:
            self._zown.sync_full(self.pc)      # the decisions read every row: whole replicas first (once per update_interval steps)
        gdist.adjust_anchor_replicated(self.pc, iteration, check_interval=opt.update_interval, success_threshold=opt.success_threshold,
                                       grad_threshold=opt.densify_grad_threshold, min_opacity=opt.min_opacity)
        if self._zown is not None:
            self._zown.ensure(self.pc)         # new anchors, new row lists (existing anchors keep their owner: z does not move)

    def _step(self, iteration: int, frame_idx: int | None = None, early: bool = True):
        for g in grid_tables(self.pc):
            g.step_cache = {}           # one binarisation of each hash table per step (gsvc_amd.encodings.GridEncoder.embeddings)
        try:
            return self._step_body(iteration, frame_idx, early)
        finally:
            for g in grid_tables(self.pc):
                g.step_cache = None

    def _step_body(self, iteration: int, frame_idx: int | None = None, early: bool = True):
        self.pc.update_learning_rate(iteration)
        if frame_idx is None:
            frame_idx = self.rng.randint(self.lo, max(self.lo, self.hi - 1))
        self._last_idx = frame_idx
        st = _Step(iteration, frame_idx, early, self.controller.render_mode)
        self._forward(st)
        self._image_terms(st)
        self._model_terms(st)
        self._combine(st)
        self._arm_exchange(st)
        self._backward(st)
        return self._finish(st)

    def _forward(self, st):
        """The four renders.  Reads iteration, frame_idx, mode; sets zown, plan, frame1, frame2, renders, batch, ovf_handle and, of the
        unbatched step, image1, image2 (attached).  Starts the replicas' overflow reduction and orders this stream behind the uploads
        of the pair's pictures."""
        pc, dist = self.pc, self._distortion
        frame_idx, mode = st.frame_idx, st.mode
        st.frame1, st.frame2 = dist.frame(self.dataset, frame_idx), dist.frame(self.dataset, frame_idx + 1)
        retain_grad = self.opt.update_until > st.iteration >= 0
        zown = st.zown = self._zown if (self._zown is not None and self.reducer.enabled) else None
        pc._zown = zown
        if zown is not None:
            zown.update_means(pc)
        if self.batched:
            # one generation pass for the 4 views (frame1 f/b, frame2 f/b), then 4 rasterizations
            plan = st.plan = self._plan if (self._plan is not None and self._plan_idx == frame_idx and self._plan_mode == mode and
                                            self._plan.matches(pc)) else None
            views = plan.frames if plan is not None else self._views(frame_idx)
            st.frame1, st.frame2 = views[0], views[2]
            with region('step.render_many'):
                st.renders = tuple(render_many(views, self.pc, self.pipe, self.background, retain_grad=retain_grad, mode=mode,
                                               dense=True, anchor_grad=self.anchor_grad, plan=plan))
            st.batch = st.renders[0].generated_gaussians.batch
            # replicas: "did any rank's instance buffer overflow" is reduced right behind the forward kernels, so that
            # the end-of-step check does not have to wait for the backward (overflow word = second int32 of a binning blob)
            st.ovf_handle = gdist.any_rank_start([r.raster_state.binning[4:8].view(torch.int32) for r in st.renders])
            self._ovf_handle = st.ovf_handle
        else:
            r1f, r1b, st.image1 = self._two_views(st.frame1, mode, retain_grad)
            r2f, r2b, st.image2 = self._two_views(st.frame2, mode, retain_grad)
            st.renders = (r1f, r1b, r2f, r2b)
        ready = getattr(self.dataset, "ready", None)
        if ready is not None:          # pictures uploaded on a copy stream (HostResidentCube): their first readers come now
            ready(frame_idx)
            ready(frame_idx + 1)

    def _image_terms(self, st):
        """The two frames' distortion, frame 1's kernels first.  Reads frame_idx, frame1, frame2, renders, image1, image2; sets terms,
        weights, const, and image1, image2 to the detached two-view frames (the batched step's are formed inside the loss kernels)."""
        dist, dev = self._distortion, self.pc.device
        r1f, r1b, r2f, r2b = st.renders
        gt1 = dist.target(self.dataset, st.frame1, st.frame_idx, dev)
        gt2 = dist.target(self.dataset, st.frame2, st.frame_idx + 1, dev)
        if self.batched:
            terms1, st.image1 = dist(r1f.rendered_image, r1b.rendered_image, gt1, frame_index=st.frame_idx)
            terms2, st.image2 = dist(r2f.rendered_image, r2b.rendered_image, gt2, frame_index=st.frame_idx + 1)
        else:
            terms1, st.image1 = dist(st.image1, None, gt1, frame_index=st.frame_idx)
            terms2, st.image2 = dist(st.image2, None, gt2, frame_index=st.frame_idx + 1)
        # the loss is a weighted sum of scalar terms: they are collected and combined with one stack + dot (instead of
        # one tiny kernel per +, *, and their backward nodes)
        st.terms = dist.image_terms(terms1, terms2)
        st.weights, st.const = dist.weights(self.opt.lambda_dssim)

    def _model_terms(self, st):
        """Regularisers, optical term, rates, hash-grid bits and mask term.  Reads frame_idx, renders, batch, plan, zown; appends to
        terms and weights (and sets ``self._mask_reg_weight``).  These terms read the generation pass's tensors and parameters, not the
        images: a dozen small launches each way, issued on the small-work stream behind the generation pass's event so that they run
        under the compositing kernels (their backward too: autograd runs a node on its forward's stream) instead of behind the image
        losses.  The step's stream waits for that stream before this returns."""
        opt, pc = self.opt, self.pc
        dev = pc.device
        batch, renders, zown, terms, weights = st.batch, st.renders, st.zown, st.terms, st.weights
        side = flow = None
        if batch is not None and batch.generated_event is not None:      # (recorded only when the batch's small_work is set)
            side = schedule.small_work_stream(dev)
            side.wait_event(batch.generated_event)
        n_image_terms = len(terms)
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            if batch is not None:
                regs = render_regs(batch.scaling, batch.neural_opacity, batch.mask, batch.seg_offsets)
                terms += [regs[0], regs[1]]
            else:
                terms += [sum(_mean_over_selected(r.scaling.prod(dim=1), r) for r in renders),
                          sum((1 - r.neural_opacity).mean() for r in renders)]
            weights += [opt.scaling_reg, opt.opacity_reg]
            if opt.optical_lambda != 0:
                flow = self.dataset.get_optical_flow(st.frame_idx)
                terms.append(calc_optical_loss(*renders, flow, self.dataset.x_min, self.dataset.y_min,
                                               self.dataset.scale, self.dataset.width, self.dataset.height, pc.n_offsets))
                weights.append(opt.optical_lambda)
            if self.controller.entropy_constrained:
                assert all(r.entropy_constrained for r in renders)
                denom = pc._anchor.shape[0] * (pc.feat_dim + 6 + 3 * pc.n_offsets)
                # sparse data-parallel exchange (_arm_exchange): the regulariser's dense gradient is added after the exchange (_add_mask_reg)
                sparse_dp = self._sparse_dp(st.plan) or zown is not None
                self._mask_reg_weight = 5e-4 if sparse_dp else 0.0
                rate_sum = batch.bit_per_param_sum if batch is not None else None
                # the renders' rates enter with one weight: their sum, when the batched generation already formed it, is one term
                terms += ([rate_sum] if rate_sum is not None else [r.bit_per_param for r in renders]) + \
                         [hash_grid_bits(pc), (zown.mask_sigmoid_mean if (zown is not None and zown.mask_sigmoid_mean is not None) else
                                               torch.mean(torch.sigmoid(pc._mask.detach() if sparse_dp else pc._mask)))]
                weights += [opt.lmbda] * (1 if rate_sum is not None else 4) + [opt.lmbda / denom, 5e-4]
        if side is not None:
            # what the terms above read of the step's stream's allocations (and saved for their backward on the small-work stream)
            schedule.record_on(side, batch.scaling, batch.neural_opacity, batch.mask, batch.world, batch.vis,
                               [g.step_cache for g in grid_tables(pc)], flow)
            main_stream = torch.cuda.current_stream(dev)
            main_stream.wait_stream(side)
            for t in terms[n_image_terms:]:
                if t.is_cuda:
                    t.record_stream(main_stream)       # allocated on the small-work stream, combined on this one

    def _combine(self, st):
        """The loss.  Reads terms, weights, const; sets loss = dot(stack(terms), weights) + const."""
        key = tuple(st.weights)
        if self._w_key != key:      # the weights change only with the training phase
            from .generate import host_values
            self._w_key, self._w = key, host_values(st.weights, self.pc.device, torch.float32)
        st.loss = torch.dot(torch.stack([t.reshape(()) for t in st.terms]), self._w) + st.const

    def _arm_exchange(self, st):
        """Data parallel: which gradients the reducer's hooks exchange in this backward, and how the per-anchor ones travel.  Reads
        mode, plan, zown; sets nothing."""
        pc, plan, zown = self.pc, st.plan, st.zown
        owned = {id(getattr(pc, n)) for n in gdist.PER_ANCHOR} if zown is not None else ()
        self.reducer.arm([p for g in pc.optimizer.param_groups for p in g["params"] if id(p) not in owned], phase=st.mode)
        use_rows = bool(self.batched and self._sparse_dp(plan))
        if use_rows:
            # the per-anchor gradients are non-zero only in the rows of this rank's distinct visible anchors: exchanged as rows
            self.reducer.set_sparse(plan.distinct, plan.distinct_cap, [pc._offset, pc._mask, pc._anchor_feat, pc._scaling])
        else:
            self.reducer.set_sparse(None, 0, [])
        if zown is not None and gdist.rank() == 0 and self._logged_exchange != "zown":
            import sys
            zown.ensure(pc)
            self._logged_exchange = "zown"
            sent, got = zown.halo_rows()
            sys.stderr.write(f"gsvc_amd.train: per-anchor tensors owned by z-range: rank 0 owns {int(zown.own_idx.shape[0])} of {int(pc._anchor.shape[0])} "
                             f"anchors, sends {sent} halo rows of gradients and returns {got} rows of parameters per step, {gdist.world_size()} ranks\n")
        elif zown is None and gdist.active() and gdist.rank() == 0 and self._logged_exchange != use_rows and plan is not None:
            import sys
            self._logged_exchange = use_rows
            sys.stderr.write(f"gsvc_amd.train: per-anchor gradient exchange = {'rows of the distinct visible anchors (cap ' + str(plan.distinct_cap) + ')' if use_rows else 'dense all-reduce'}"
                             f" at {int(pc._anchor.shape[0])} anchors, {gdist.world_size()} ranks\n")

    def _early_plan_pays(self, st):
        """Whether this backward updates ``_scaling`` / ``_mask`` and queues the next step's plan from inside (``_early_tail``).  Reads
        iteration, early, mode, zown, batch."""
        opt, pc = self.opt, self.pc
        return bool(st.early and self.batched and self.prefetch and pc._anchor.is_cuda
                    and (not gdist.active() or (self.reducer.enabled and self.reducer._order is not None and st.zown is None))
                    and not self.anchor_grad      # a trained anchor tensor moves behind the early plan's visibility test
                    and st.mode is not None and st.iteration < opt.iterations and not self.controller.gaussian_adjust_anchor
                    and isinstance(pc.optimizer, FusedAdam) and not switches.NO_EARLY_PLAN
                    and pc._scaling.requires_grad and pc._mask.requires_grad
                    # it pays when the GPU, not the host, bounds the step (the hook's work costs ~1 ms of host time more on the
                    # autograd thread than at the end of the step: a 6 k-row step went 8.3 -> 9.7 ms, the 200 k-row step 11.95 -> 11.3)
                    and (switches.EARLY_PLAN or st.batch.gpu_bound))

    def _backward(self, st):
        """The backward and the gradients' exchange.  Reads loss, renders, batch, mode, zown and what ``_early_plan_pays`` reads; sets nothing.
        The hook below holds ``self``, the renders, the tensors it waits for and its counter — not the step record."""
        pc, renders, batch, loss, zown = self.pc, st.renders, st.batch, st.loss, st.zown
        dev = pc.device
        handles = []
        if self._early_plan_pays(st):
            # STE_ENTROPY renders from detached attributes (reference guassian.py:205-207): _scaling receives no gradient there,
            # is not changed by the step, and its hook would never run
            waited = [pc._mask] if st.mode == GenerateMode.TRAININ_STE_ENTROPY else [pc._scaling, pc._mask]
            pending = [len(waited)]

            def arrived(_p):
                pending[0] -= 1
                if pending[0] == 0:
                    self._early_tail(renders, waited)
            handles = [p.register_post_accumulate_grad_hook(arrived) for p in waited]
        try:
            # a GPU-bound step (the one that uses the small-work stream) also sends the chain networks' weight gradients to their own
            # stream, and waits for both streams behind the backward; a host-bound one would only pay for the events and the allocator's
            # stream records (configs[3]: +0.2 ms of host time)
            with region('step.backward'), (schedule.backward_streams(dev, self._chain_params) if batch is not None and batch.small_work
                                           else contextlib.nullcontext()):
                loss.backward()
        finally:
            for h in handles:
                h.remove()
        done = getattr(self.dataset, "step_done", None)
        if done is not None:
            done()      # every reader of the ground-truth slots (image losses, optical term — forward and backward, this stream and the
                        # small-work stream, which this one has just waited for) is queued: the slots' next upload may start behind here
        with region('step.reducer_finish'):
            self.reducer.finish()
            if zown is not None:
                zown.exchange_grads(pc, self._zown_names(st.mode))
            self._add_mask_reg()

    def _finish(self, st):
        """Counters and the overflow verdict (None: the step is to be repeated), densification statistics, anchor adjustment,
        optimizer, and the graph-free StepOutput.  Reads iteration, frame_idx, mode, zown, renders, ovf_handle, loss, image1, image2."""
        opt, pc, renders, zown = self.opt, self.pc, st.renders, st.zown
        if self.batched:
            # the only host synchronisation of the step after the visibility test: the 4 renders' instance counters
            with region('step.resolve_counters'):
                _, overflowed = resolve_deferred([r.raster_state for r in renders])
            if gdist.any_rank_finish(st.ovf_handle, overflowed):      # replicas repeat the step together (their collectives must pair up)
                return None
            for r in renders:
                r.num_rendered = r.raster_state.counters()[0]
        with torch.no_grad():
            if self.controller.gaussian_statis:
                if self.batched:
                    with region('step.statis'):
                        pc.training_statis_many(renders)
                else:
                    for r in renders:
                        pc.training_statis(r)
            if self.controller.gaussian_adjust_anchor:
                self._adjust_anchor(st.iteration)
            if self.controller.clean_denorm:
                pc.opacity_accum = pc.offset_gradient_accum = pc.offset_denom = None
            if st.iteration < opt.iterations:
                with region('step.optimizer'):
                    pc.optimizer.step()
                    pc.optimizer.zero_grad(set_to_none=True)
                    if zown is not None:
                        zown.refresh_params(pc, self._zown_names(st.mode))
        active = sum(r.active_gaussains for r in renders)
        _release_graph(renders)      # at every size: a StepOutput never carries the step's autograd graph (see _release_graph)
        return StepOutput(loss=st.loss.detach(), image1=st.image1, image2=st.image2, renders=renders,
                          active_gaussians=active, frame_idx=st.frame_idx)
