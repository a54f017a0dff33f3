"""Drop-in for ``diff_gaussian_rasterization.cuda_ortho_gaussian_rasterizer`` (external CUDA extension of
GSVC, reference README.md:52) backed by the gfx950 HIP kernels of ``csrc/raster_{fwd,bwd}.hip``.

Mirrors the surface GSVC uses:
  * ``GaussianRasterizationSettings(image_height, image_width, x_min, y_min, scale, threshold, bg,
    scale_modifier, viewmatrix, sh_degree, campos, prefiltered, debug)`` — keyword construction,
    reference ortho_gaussian_renderer/renderer.py:63-83;
  * ``GaussianRasterizer(raster_settings=...)(means3D=, means2D=, shs=, colors_precomp=, opacities=,
    scales=, rotations=, cov3D_precomp=) -> (image[3,H,W], radii[P], num_rendered)``, renderer.py:85-98;
  * ``GaussianRasterizer.visible_filter(means3D=, scales=, rotations=, cov3D_precomp=) -> radii``,
    reference ortho_gaussian_renderer/preprocess.py:99-104;
  * an autograd node: ``means2D.grad`` receives the screen-space gradient (renderer.py:37-42,
    scene/gaussian_model.py:1311).

Both colour sources and both covariance sources of the lineage are built:
  * ``shs`` [P, K, 3] (with ``colors_precomp=None``): colours from the real spherical harmonics of degree
    ``raster_settings.sh_degree`` (0..3, (degree+1)^2 <= K) evaluated in the kernel at
    dir = normalize(means3D - raster_settings.campos), or at the view's constant axis under
    ``flags & GSVC_RASTER_SH_VIEW_AXIS`` (DESIGN.md "Raster spec"); the backward returns dL/dshs and adds the
    gradient through dir to dL/dmeans3D;
  * ``cov3D_precomp`` [P, 6] = xx, xy, xz, yy, yz, zz (with ``scales``/``rotations`` None), used as given
    (``scale_modifier`` is not applied, as in the lineage); the backward returns dL/dcov3D_precomp.

One host path serves every call: one autograd function (``_RasterizeGaussians``), one foreign call in ``raster_forward`` and one
in ``_raster_backward`` (which the batched ``_RasterizeMany`` shares), with the entry point chosen by one rule,
    pair -> gsvc_raster_forward_pair;  else maps -> _forward_aux / _backward_aux;  else shs or cov3D_precomp -> _forward_ex /
    _backward_ex;  else gsvc_raster_forward / _backward
(``visible_filter``: cov3D_precomp -> _visible_filter_ex, else gsvc_raster_visible_filter).  GSVC itself always passes
colors_precomp + scales/rotations without maps, so its calls keep the original entry points and their kernels.

``forward(..., return_depth=True and / or return_alpha=True)`` also returns the two per-pixel maps of the same composite,
``depth`` [1, H, W] = sum_i w_i z_i (z_i the view-space z, not normalised: divide by ``alpha`` for the mean depth) and
``alpha`` [1, H, W] = 1 - T_final, as ``(image, radii, num_rendered, depth, alpha)`` (None for a map not asked for), with
their backward (gsvc_raster_forward_aux / _backward_aux, any colour / covariance source).  Single view only.

Error behaviour follows the 3DGS lineage: both/neither of shs and colors_precomp, or of scales/rotations
and cov3D_precomp, raise ``Exception``.  SH colours are single-view only (not in raster_forward(pair=True) /
rasterize_many).
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib, schedule


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    x_min: float
    y_min: float
    scale: float
    threshold: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    sh_degree: int = 0
    campos: Optional[torch.Tensor] = None
    prefiltered: bool = False
    debug: bool = False
    # not fields of the reference's settings: the convention switches of include/gsvc_hip.h (GSVC_RASTER_*, 0 = DESIGN.md's
    # raster spec) and the low-pass added to the 2-D covariance (0 = the default 0.3), see INTEGRATION.md
    flags: int = 0
    low_pass: float = 0.0


def _host_floats(t, n):
    if isinstance(t, torch.Tensor):
        a = t.detach().to("cpu", torch.float32).contiguous().view(-1).numpy()  # syncs if t lives on the GPU
    else:
        a = np.asarray(t, dtype=np.float32).reshape(-1)
    if a.size != n:
        raise ValueError(f"expected {n} floats, got {a.size}")
    return a


def settings_to_c(rs: GaussianRasterizationSettings) -> _lib.RasterSettingsC:
    s = _lib.RasterSettingsC()
    s.image_height, s.image_width = int(rs.image_height), int(rs.image_width)
    s.x_min, s.y_min, s.scale = float(rs.x_min), float(rs.y_min), float(rs.scale)
    s.threshold, s.scale_modifier = float(rs.threshold), float(rs.scale_modifier)
    s.bg[:] = _host_floats(rs.bg, 3).tolist()
    s.viewmatrix[:] = _host_floats(rs.viewmatrix, 16).tolist()
    s.flags, s.low_pass = int(getattr(rs, "flags", 0)), float(getattr(rs, "low_pass", 0.0))
    return s


def _as_f32(t: Optional[torch.Tensor], name: str) -> Optional[torch.Tensor]:
    if t is None:       # an input a source replaces, a gradient nothing was computed from
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _inputs_f32(means3D, colors, opacities, scales, rotations):
    return (_as_f32(means3D, "means3D"), _as_f32(colors, "colors_precomp"), _as_f32(opacities, "opacities"),
            _as_f32(scales, "scales"), _as_f32(rotations, "rotations"))


class RasterState:
    """Opaque state of one forward (geom / binning / image blobs) kept for backward and inspection."""

    def __init__(self, cs, P, max_instances, geom, binning, image_state, radii):
        self.cs, self.P, self.max_instances = cs, P, max_instances
        self.geom, self.binning, self.image_state, self.radii = geom, binning, image_state, radii
        self._counters = self._listed = None
        self._host = self._event = None     # early asynchronous read-back of the counters (raster_forward, sync=False)

    def counters(self):
        """(num_rendered, overflow, num_visible, max_tile_len) — one 16-byte D2H copy (synchronises), cached."""
        if self._counters is None:
            c = self.binning[:32].view(torch.int32).tolist()
            self._counters, self._listed = tuple(int(v) for v in c[:4]), int(c[7])
        return self._counters

    def tile_lists(self):
        """(tile_offsets[T+1], point_list[instances listed]) as int32 tensors (views into the binning blob).  The lists' length is
        tile_offsets[T]: num_rendered counts the 3-sigma rectangles' tiles, which is more under GSVC_RASTER_TIGHT_BINNING."""
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(_lib.lib().gsvc_raster_binning_layout(C.byref(self.cs), self.P, self.max_instances, C.byref(a), C.byref(b)),
                   "gsvc_raster_binning_layout")
        H, W = self.cs.image_height, self.cs.image_width
        T = ((H + 15) // 16) * ((W + 15) // 16)
        if self.counters()[1]:
            raise _lib.GsvcError("tile_lists: the forward overflowed its instance buffer (no lists were written)")
        off = self.binning[a.value:a.value + 4 * (T + 1)].view(torch.int32)
        n = int(off[T])
        pl = self.binning[b.value:b.value + 4 * n].view(torch.int32)
        return off, pl

    def listed_instances(self) -> int:
        """(tile, Gaussian) instances the tile lists hold = tile_offsets[T]: what the sort, the compositing kernels and the backward's
        rows work on.  Equal to num_rendered for the 3-sigma lists, fewer under GSVC_RASTER_TIGHT_BINNING (one 4-byte copy: synchronises)."""
        if self._listed is None:          # (the counters' read-back carries it: gsvc_raster_counters.reserved[2])
            self.counters()
        return self._listed

    def image_aux(self):
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(_lib.lib().gsvc_raster_image_layout(C.byref(self.cs), C.byref(a), C.byref(b)), "gsvc_raster_image_layout")
        H, W = self.cs.image_height, self.cs.image_width
        gy, gx = (H + 15) // 16, (W + 15) // 16
        n = gy * gx * 256

        def rows(t):      # the blob keeps them tile-major [tile_y, tile_x, quad_y, quad_x, lane_y, lane_x]
            return t.view(gy, gx, 2, 2, 8, 8).permute(0, 2, 4, 1, 3, 5).reshape(gy * 16, gx * 16)[:H, :W].contiguous()
        fT = rows(self.image_state[a.value:a.value + 4 * n].view(torch.float32))
        nc = rows(self.image_state[b.value:b.value + 4 * n].view(torch.int32))
        return fT, nc


_capacity_hint = {}


def raster_forward(cs: _lib.RasterSettingsC, means3D, colors, opacities, scales, rotations, max_instances=None,
                   sync=True, pair=False, readback=False, radii_out=None, side_stream=None, sources=None, maps_out=None):
    """Launch the forward pipeline.  Returns (image, radii, state).  With ``sync`` the instance counters
    are read back (16 B) and the call is repeated with a larger instance capacity if it overflowed; without
    it the caller must check ``state.counters()[1]`` itself (``readback``: the counters' copy to the host is queued right
    behind the forward, for resolve_deferred()).  ``pair=True`` returns the two-view frame
    (render(view) + flip(render(opposite view))) / 2 from one pass (inference only, see gsvc_raster_forward_pair).
    ``sources`` (a RasterSourcesC: SH colours and / or a precomputed covariance, single view only) selects
    gsvc_raster_forward_ex; ``colors`` / ``scales`` + ``rotations`` are then None where it replaces them.  ``maps_out`` (depth,
    alpha): [1, H, W] float32 tensors or None, written by gsvc_raster_forward_aux (single view; ``sources`` may be None).
    One foreign call: ``pair`` -> _pair, else ``maps_out`` -> _aux, else ``sources`` -> _ex, else gsvc_raster_forward."""
    if pair and maps_out is not None:
        raise ValueError("raster_forward: the depth / alpha maps serve the single-view forward only")
    if pair and sources is not None:
        raise ValueError("raster_forward: SH colours / cov3D_precomp serve the single-view forward only")
    # the entry point and what its signature has beyond the plain one's: the sources (_ex, _aux), the two maps (_aux)
    p = _lib.ptr
    suffix = "_pair" if pair else "_aux" if maps_out is not None else "_ex" if sources is not None else ""
    name = "gsvc_raster_forward" + suffix
    src_arg = (None if sources is None else C.byref(sources),) if suffix in ("_ex", "_aux") else ()
    maps_arg = (p(maps_out[0]), p(maps_out[1])) if suffix == "_aux" else ()
    L = _lib.lib()
    P = int(means3D.shape[0])
    dev = means3D.device
    H, W = cs.image_height, cs.image_width
    key = (H, W)
    if max_instances is None:
        max_instances = max(_capacity_hint.get(key, 0), 4 * P, 1 << 16)
    # side_stream (a torch.cuda.Stream the caller has made wait for the inputs, and waits for afterwards): the kernels go there;
    # every buffer is still allocated on the CURRENT stream's pool (the caller's join orders any reuse behind the side work)
    stream = _lib.current_stream(dev) if side_stream is None else C.c_void_p(side_stream.cuda_stream)
    while True:
        sizes = _lib.RasterSizesC()
        _lib.check(L.gsvc_raster_sizes_query(C.byref(cs), P, max_instances, C.byref(sizes)), "gsvc_raster_sizes_query")
        geom = torch.empty(sizes.geom_bytes, dtype=torch.uint8, device=dev)
        binning = torch.empty(sizes.binning_bytes, dtype=torch.uint8, device=dev)
        image_state = torch.empty(sizes.image_bytes, dtype=torch.uint8, device=dev)
        image = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        radii = radii_out if radii_out is not None else torch.empty(P, dtype=torch.int32, device=dev)
        _lib.check(getattr(L, name)(C.byref(cs), P, max_instances, p(means3D), p(colors), p(opacities), p(scales), p(rotations),
                                    *src_arg, p(image), p(radii), p(geom), p(binning), p(image_state), *maps_arg, stream), name)
        state = RasterState(cs, P, max_instances, geom, binning, image_state, radii)
        if not sync and readback:
            # the counters are final once the forward kernels have run: their 16 bytes start travelling to the host
            # now, behind the forward only, so that resolve_deferred() later waits for THIS copy and not for
            # everything queued after it (the whole backward of a fitting step)
            state._host = torch.empty(8, dtype=torch.int32, pin_memory=True)
            src = binning[:32].view(torch.int32)
            with torch.cuda.stream(side_stream) if side_stream is not None else contextlib.nullcontext():
                state._host.copy_(src, non_blocking=True)
                state._event = torch.cuda.Event()
                state._event.record()
        if not sync:
            return image, radii, state
        n, overflow, _, _ = state.counters()
        n = state._listed or n          # the LISTS' length decides the capacity (shorter than num_rendered under tight binning: ADVICE r05)
        if not overflow:
            _capacity_hint[key] = max(_capacity_hint.get(key, 0), int(n * 1.25) + 1024)
            return image, radii, state
        max_instances = int(n * 1.25) + 1024


def resolve_deferred(states):
    """Read back, with ONE host synchronisation, the instance counters of forwards launched with ``sync=False``.
    Returns (num_rendered list, overflowed: bool); on overflow the capacity hint is raised so that repeating the
    forwards succeeds — their images (and anything computed from them) must be discarded."""
    if not states:
        return [], False
    if all(getattr(st, "_event", None) is not None for st in states):
        for st in states:
            schedule.blocked_wait(st._event)      # (what the host blocks here is the GPU's lead over it: Trainer's bound detector)
        host = [st._host.tolist() for st in states]
    else:
        host = torch.stack([st.binning[:32].view(torch.int32) for st in states]).tolist()
    over = False
    for st, c in zip(states, host):
        st._counters, st._listed = tuple(int(v) for v in c[:4]), int(c[7])
        key = (st.cs.image_height, st.cs.image_width)
        _capacity_hint[key] = max(_capacity_hint.get(key, 0), int((c[7] or c[0]) * 1.25) + 1024)
        over = over or bool(c[1])
    return [c[0] for c in host], over


def backward_scratch_floats(P: int, max_instances: int) -> int:
    """Floats of scratch gsvc_raster_backward needs (one 64-byte row of partial sums per instance)."""
    return int(_lib.lib().gsvc_raster_backward_scratch_bytes(int(P), int(max_instances))) // 4


def _sources_c(shs, sh_degree, campos, cov3D):
    """gsvc_raster_sources for the tensors given (None: that source is not used)."""
    src = _lib.RasterSourcesC()
    src.shs, src.cov3D = _lib.ptr(shs), _lib.ptr(cov3D)
    if shs is not None:
        src.sh_degree, src.sh_coeffs = int(sh_degree), int(shs.shape[1])
        src.campos[:] = list(campos)
    return src


def _grad_buffers(n, dev):
    """The six gradient tensors of n Gaussians: means3D, means2D, colors, opacities, scales, rotations."""
    return tuple(torch.empty(n, k, device=dev) for k in (3, 3, 3, 1, 3, 4))


def _backward_scratch(st, dev):
    return torch.empty(backward_scratch_floats(st.P, st.max_instances), device=dev)


def _raster_backward(st, inputs, g, grads, scratch, stream, src=None, src_grads=(None, None), map_grads=None):
    """The backward of the forward ``st``, queued on ``stream``: ``inputs`` (means3D, colors, opacities, scales, rotations: the
    forward's, None where a source replaces one) and the six ``grads`` are the render's own rows, ``g`` its image gradient,
    ``scratch`` its partial-sum rows.  One foreign call, chosen by raster_forward's rule: ``map_grads`` (dL/ddepth, dL/dalpha,
    each a tensor or None) -> gsvc_raster_backward_aux, else ``src`` -> _ex (both with ``src_grads`` = dL/dshs, dL/dcov3D),
    else gsvc_raster_backward."""
    p = _lib.ptr
    suffix = "_aux" if map_grads is not None else "_ex" if src is not None else ""
    name = "gsvc_raster_backward" + suffix
    args = [C.byref(st.cs), st.P, st.max_instances, *map(p, inputs)]
    if suffix:
        args.append(None if src is None else C.byref(src))
    args += (p(st.radii), p(st.geom), p(st.binning), p(st.image_state), p(g))
    if map_grads is not None:
        args += map(p, map_grads)
    args += map(p, grads)
    if suffix:
        args += map(p, src_grads)
    _lib.check(getattr(_lib.lib(), name)(*args, p(scratch), stream), name)


class _RasterizeGaussians(torch.autograd.Function):
    """One rasterization: outputs (image, radii, depth or None, alpha or None).  colors_precomp + scales / rotations without maps
    take gsvc_raster_forward / _backward; SH colours and / or a precomputed 3-D covariance (``shs`` / ``cov3D``, the input they
    replace is None) the _ex entry points; ``maps`` = (depth?, alpha?) not (False, False) the _aux ones, with any sources."""

    @staticmethod
    def forward(ctx, means3D, means2D, colors, opacities, scales, rotations, shs, cov3D, cs, sh_degree, campos, holder, sync=True,
                maps=(False, False)):
        means3D, colors, opacities, scales, rotations = _inputs_f32(means3D, colors, opacities, scales, rotations)
        shs, cov3D = _as_f32(shs, "shs"), _as_f32(cov3D, "cov3D_precomp")
        if shs is not None and (shs.dim() != 3 or shs.shape[0] != means3D.shape[0] or shs.shape[2] != 3):
            raise ValueError(f"shs must be [P, coefficients, 3], got {tuple(shs.shape)}")
        if cov3D is not None and tuple(cov3D.shape) != (means3D.shape[0], 6):
            raise ValueError(f"cov3D_precomp must be [P, 6], got {tuple(cov3D.shape)}")
        src = _sources_c(shs, sh_degree, campos, cov3D) if shs is not None or cov3D is not None else None
        H, W = cs.image_height, cs.image_width
        aux = any(maps)
        depth, alpha = (torch.empty(1, H, W, dtype=torch.float32, device=means3D.device) if want else None for want in maps)
        image, radii, state = raster_forward(cs, means3D, colors, opacities, scales, rotations, sync=sync, readback=not sync,
                                             sources=src, maps_out=(depth, alpha) if aux else None)
        ctx.state, ctx.src, ctx.aux = state, src, aux
        ctx.save_for_backward(means3D, colors, opacities, scales, rotations, shs, cov3D)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        holder["state"] = state
        return image, radii, depth, alpha

    @staticmethod
    def backward(ctx, grad_image, _grad_radii, grad_depth=None, grad_alpha=None):
        means3D, colors, opacities, scales, rotations, shs, cov3D = ctx.saved_tensors
        st = ctx.state
        P = st.P
        dev = means3D.device
        H, W = st.cs.image_height, st.cs.image_width
        # (gradients are not materialised: an output the loss does not use arrives as None; a map's None is a NULL pointer)
        g = _as_f32(grad_image, "grad_image") if grad_image is not None else torch.zeros(3, H, W, device=dev)
        map_grads = (_as_f32(grad_depth, "grad_depth"), _as_f32(grad_alpha, "grad_alpha")) if ctx.aux else None
        grads = _grad_buffers(P, dev)
        dsh = torch.empty_like(shs) if shs is not None else None
        dcov = torch.empty(P, 6, device=dev) if cov3D is not None else None
        _raster_backward(st, (means3D, colors, opacities, scales, rotations), g, grads, _backward_scratch(st, dev),
                         _lib.current_stream(dev), ctx.src, (dsh, dcov), map_grads)
        d3, d2, dc, do, ds, dq = grads
        return (d3, d2, dc if colors is not None else None, do, ds if scales is not None else None,
                dq if rotations is not None else None, dsh, dcov, None, None, None, None, None, None)


class _RasterizeMany(torch.autograd.Function):
    """R rasterizations of consecutive row ranges of ONE set of Gaussian tensors (the un-compacted renders of a fitting step are
    slices of the batch the generation pass produced): the forward launches the R pipelines on the ranges in place, the backward
    writes every render's gradients straight into its rows of batch-sized tensors.  As R separate autograd functions the batch
    tensors were split on the way in and their six gradients concatenated on the way back (six cat launches, 84 us per step),
    with a zero-filled means2D leaf and a radii tensor per render."""

    @staticmethod
    def forward(ctx, means3D, means2D, colors, opacities, scales, rotations, cs_list, bounds, holder):
        means3D, colors, opacities, scales, rotations = _inputs_f32(means3D, colors, opacities, scales, rotations)
        N = int(means3D.shape[0])
        radii = torch.empty(N, dtype=torch.int32, device=means3D.device)
        images, states = [], []
        # the renders are independent pipelines of dependent kernels (bin, scatter, sort, composite): dealt to two side streams,
        # one render's kernel boundaries and tails are filled by the other's kernels
        side = schedule.raster_streams(means3D.device, len(cs_list))
        main = torch.cuda.current_stream(means3D.device)
        for sd in side:
            sd.wait_stream(main)
        for r, cs in enumerate(cs_list):
            a, b = bounds[r], bounds[r + 1]
            img, _, st = raster_forward(cs, means3D[a:b], colors[a:b], opacities[a:b], scales[a:b], rotations[a:b], sync=False,
                                        readback=True, radii_out=radii[a:b], side_stream=side[r % len(side)] if side else None)
            images.append(img)
            states.append(st)
        for sd in side:
            main.wait_stream(sd)
        ctx.states, ctx.bounds = states, tuple(bounds)
        ctx.save_for_backward(means3D, colors, opacities, scales, rotations)
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        holder["states"] = states
        return (*images, radii)

    @staticmethod
    def backward(ctx, *grad_images):
        inputs = ctx.saved_tensors          # means3D, colors, opacities, scales, rotations
        N, dev = inputs[0].shape[0], inputs[0].device
        grads = _grad_buffers(N, dev)
        side = schedule.raster_streams(dev, len(ctx.states))
        main = torch.cuda.current_stream(dev)
        # everything the side streams read is produced / allocated on the main stream BEFORE the fork: an image gradient that is
        # not contiguous fp32 (an expanded gradient of images[r].sum(), autocast) is converted by a copy kernel on main, and the
        # scratch rows are allocated there — converting after the fork left the side stream's backward reading the copy's
        # destination with nothing ordering the two
        gs = [_as_f32(g, "grad_image") for g in grad_images[:len(ctx.states)]]
        scratches = [None if g is None else _backward_scratch(st, dev) for g, st in zip(gs, ctx.states)]  # alive until the join below
        for r, g in enumerate(gs):
            if g is None:           # a render nothing was computed from: its Gaussians get no gradient
                a, b = ctx.bounds[r], ctx.bounds[r + 1]
                for t in grads:
                    t[a:b].zero_()
        for sd in side:
            sd.wait_stream(main)
        for r, st in enumerate(ctx.states):
            a, b = ctx.bounds[r], ctx.bounds[r + 1]
            if gs[r] is None:
                continue
            stream = C.c_void_p(side[r % len(side)].cuda_stream) if side else _lib.current_stream(dev)
            _raster_backward(st, [t[a:b] for t in inputs], gs[r], [t[a:b] for t in grads], scratches[r], stream)
        for sd in side:
            main.wait_stream(sd)
        del scratches, gs
        return (*grads, None, None, None)


def rasterize_many(cs_list, bounds, means3D, means2D, colors, opacities, scales, rotations):
    """(images [R], radii [N] int32, states [R]) of R un-synchronised rasterizations over the row ranges ``bounds`` (R + 1
    offsets) of the given tensors; ``means2D`` is the [N, 3] leaf whose .grad receives the screen-space gradients.  The caller
    resolves the instance counters with resolve_deferred(states)."""
    holder = {}
    out = _RasterizeMany.apply(means3D, means2D, colors, opacities, scales, rotations, list(cs_list), list(bounds), holder)
    return list(out[:-1]), out[-1], holder["states"]


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings
        self._cs = None
        self.last_state: Optional[RasterState] = None
        self.deferred = False   # True: forward() does not read the counters back (third return value = RasterState)
        self._campos_host = None

    def _c_settings(self):
        if self._cs is None:
            self._cs = settings_to_c(self.raster_settings)
        return self._cs

    def _campos(self):
        """settings.campos as three host floats (read once: a tensor on the GPU costs a synchronising copy)."""
        if self._campos_host is None:
            rs = self.raster_settings
            if rs.campos is None:
                if not (int(getattr(rs, "flags", 0)) & _lib.RASTER_SH_VIEW_AXIS):
                    raise ValueError("SH colours need raster_settings.campos (or flags & GSVC_RASTER_SH_VIEW_AXIS)")
                self._campos_host = (0.0, 0.0, 0.0)
            else:
                self._campos_host = tuple(float(v) for v in _host_floats(rs.campos, 3))
        return self._campos_host

    def visible_filter(self, means3D, scales=None, rotations=None, cov3D_precomp=None):
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        with torch.no_grad():
            m, s, q = _as_f32(means3D, "means3D"), _as_f32(scales, "scales"), _as_f32(rotations, "rotations")
            P = int(m.shape[0])
            name, src_arg = "gsvc_raster_visible_filter", ()
            if cov3D_precomp is not None:
                cov = _as_f32(cov3D_precomp, "cov3D_precomp")
                if tuple(cov.shape) != (P, 6):
                    raise ValueError(f"cov3D_precomp must be [P, 6], got {tuple(cov.shape)}")
                src = _sources_c(None, 0, None, cov)        # (keeps cov alive over the call)
                name, src_arg = "gsvc_raster_visible_filter_ex", (C.byref(src),)
            radii = torch.empty(P, dtype=torch.int32, device=m.device)
            _lib.check(getattr(_lib.lib(), name)(C.byref(self._c_settings()), P, _lib.ptr(m), _lib.ptr(s), _lib.ptr(q), *src_arg,
                                                 _lib.ptr(radii), _lib.current_stream(m.device)), name)
        return radii

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, *, return_depth=False, return_alpha=False):
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        holder = {}
        maps = (bool(return_depth), bool(return_alpha))
        image, radii, depth, alpha = _RasterizeGaussians.apply(
            means3D, means2D, colors_precomp, opacities, scales, rotations, shs, cov3D_precomp, self._c_settings(),
            int(self.raster_settings.sh_degree), self._campos() if shs is not None else None, holder, not self.deferred, maps)
        self.last_state = holder["state"]
        # counters stay on the device under `deferred`: the caller resolves them with resolve_deferred()
        third = self.last_state if self.deferred else self.last_state.counters()[0]
        if any(maps):
            return image, radii, third, depth, alpha
        return image, radii, third
