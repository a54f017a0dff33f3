"""The rasterizer kernels against float64, per element.

gsvc_raster_forward / _aux / _pair and gsvc_raster_backward / _aux are called through ctypes on test-owned buffers, every output and
the backward's `scratch` pre-filled (with a tail pad) with a NaN payload no input produces.  What is looked at: the float fields of
GeomRec, the image / final_T / n_contrib / maps of k_blend, the two-view frame, every partial-sum row k_blend_bwd_tile writes
(located by GeomRec::goff + the tile's place in the rectangle), k_gaussian_bwd on those rows alone, and the six gradients of the
autograd path per Gaussian.  References: tests/_raster_kernel_refs.py (pinned by tests/test_raster_kernel_refs_cpu.py) fed with the
fp32 numbers the kernels themselves stored, cast up.

Rule, wherever a float is compared: e = max |got - ref64| / scale per element (scale = that element's own sum of absolute terms),
no element excluded other than borderline pixels (the backward tests zero dL there), and e_kernel <= 4 e32 + 4 eps32, e32 being the
NumPy float32 run of the form the kernel path uses with the float64 decisions.  A path that mixes the two forms chunk by chunk
(scene L without the probe instantiation) takes the larger of the two e32: every element went through one or the other.
GSVC_PRINT_ERRORS=1 prints e_kernel, e32 and the C oracle's own error for every case.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from gsvc_amd import _lib
from tests import _raster_kernel_refs as K

pytestmark = pytest.mark.gpu

BLACK, BG = (0.0, 0.0, 0.0), (0.3, 0.1, 0.6)
NAN_BITS = 0x7FC0DEAD          # a quiet NaN with a payload: no arithmetic on the inputs produces these bits
PAD = 64                       # floats behind every output
TAIL_ROWS = 7                  # rows of scratch beyond the instances listed
IN = ("means3D", "colors", "opacities", "scales", "rotations")


def _nan_buf(n):
    return torch.full((n + PAD,), NAN_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def _untouched(t):
    return (t.view(torch.int32) == NAN_BITS).cpu().numpy()


def _report(tag, e_k, e32, e_or=None):
    if os.environ.get("GSVC_PRINT_ERRORS"):
        print(f"RASTER_ERR {tag}: e_kernel {e_k:.3e}  e32 {e32:.3e}  oracle " + ("-" if e_or is None else f"{e_or:.3e}"))


def _assert_rule(tag, e_k, e32, e_or=None):
    _report(tag, e_k, e32, e_or)
    assert np.isfinite(e32), (tag, e32)            # an infinite e32 would let anything pass
    assert K.within_rule(e_k, e32), (tag, e_k, e32)


def _e32(runs, ref, scale, unsafe):
    """The rule's e32 from the float32 runs {form: values} of the forms a kernel path takes.  One form: its error.  Both (scene L
    outside the probe instantiation: the kernel picks the form chunk by chunk): rows of a Gaussian whose conic fails the
    polynomial's test (`unsafe`) always take the literal loops and are held to the literal run; the other rows take either, and
    are held to the larger of the two errors of that element."""
    e = {form: K.rule_errors(v, ref, scale) for form, v in runs.items()}
    if len(e) == 1:
        return float(next(iter(e.values())).max())
    both = np.maximum(e["literal"], e["poly"])
    return float(max(e["literal"][unsafe].max(initial=0.0), both[~unsafe].max(initial=0.0)))


def _c_settings(s, bg, view="viewmatrix", flags=None):
    from gsvc_amd.rasterizer import GaussianRasterizationSettings, settings_to_c
    return settings_to_c(GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], x_min=s["x_min"], y_min=s["y_min"], scale=s["scale"], threshold=s["threshold"],
        bg=torch.tensor(bg, dtype=torch.float32), scale_modifier=s["scale_modifier"], viewmatrix=torch.tensor(s[view]), sh_degree=0,
        campos=torch.tensor([0.0, 0.0, s["z_cam"]]), prefiltered=False, debug=False,
        flags=s.get("flags", 0) if flags is None else flags, low_pass=s.get("low_pass", 0.0)))


def _call_forward(cs, d, cap, entry="", sources=None):
    """One foreign call of gsvc_raster_forward{,_ex,_aux,_pair} on NaN-filled outputs.  Returns (state, image, depth, alpha) tensors
    (the outputs with their pads).  `sources` (a RasterSourcesC holding cov3D): scales and rotations are then not passed."""
    from gsvc_amd.rasterizer import RasterState
    L, p = _lib.lib(), _lib.ptr
    P, H, W = int(d["means3D"].shape[0]), cs.image_height, cs.image_width
    sizes = _lib.RasterSizesC()
    _lib.check(L.gsvc_raster_sizes_query(C.byref(cs), P, cap, C.byref(sizes)), "gsvc_raster_sizes_query")
    geom, binning, image_state = (torch.zeros(int(n), dtype=torch.uint8, device="cuda")
                                  for n in (sizes.geom_bytes, sizes.binning_bytes, sizes.image_bytes))
    image, depth, alpha = _nan_buf(3 * H * W), _nan_buf(H * W), _nan_buf(H * W)
    radii = torch.zeros(P, dtype=torch.int32, device="cuda")
    name = "gsvc_raster_forward" + entry
    src = (None if sources is None else C.byref(sources),) if entry in ("_aux", "_ex") else ()
    sr = (None, None) if sources is not None else (p(d["scales"]), p(d["rotations"]))
    maps = (p(depth), p(alpha)) if entry == "_aux" else ()
    _lib.check(getattr(L, name)(C.byref(cs), P, cap, p(d["means3D"]), p(d["colors"]), p(d["opacities"]), *sr,
                                *src, p(image), p(radii), p(geom), p(binning), p(image_state), *maps,
                                _lib.current_stream(torch.device("cuda"))), name)
    torch.cuda.synchronize()
    return RasterState(cs, P, cap, geom, binning, image_state, radii), image, depth, alpha


def _geom_records(st):
    """GeomRec[P] as [P, 16] uint32 (float fields through .view(np.float32))."""
    return st.geom[: st.P * 64].view(torch.int32).view(st.P, 16).cpu().numpy().view(np.uint32)


def _s16(v):
    return (v & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64)


class _Fwd:
    """One scene through the oracle, the GPU forward (twice) and the references, shared by the tests of this file."""

    def __init__(self, name, bg, aux=False, view="viewmatrix", cov=False):
        import oracle
        oracle.build()
        self.name, self.bg, self.aux, self.view = name, bg, aux, view
        sc = self.sc = K.scene(name)
        s = self.s = sc["settings"]
        self.st = dict(s, bg=bg)
        self.H, self.W, self.P = s["H"], s["W"], sc["means3D"].shape[0]
        self.fw = fw = K.oracle_forward(oracle, sc, bg=bg, view=view)
        self.cap = fw.num_rendered + TAIL_ROWS
        self.d = {k: torch.tensor(sc[k], device="cuda").contiguous() for k in IN}
        self.d["opacities"] = self.d["opacities"].view(-1).contiguous()
        self.cs = _c_settings(s, bg, view)
        # cov: the 3-D covariance as a source (gsvc_raster_forward_ex), the float32 numbers the scale / rotation call forms itself
        self.cov = self.sources = None
        if cov:
            from gsvc_amd.rasterizer import _sources_c
            assert not aux
            self.cov = K.cov3d_ref(sc["scales"], sc["rotations"], s, np.float32)
            self.d["cov3D"] = torch.tensor(self.cov, device="cuda").contiguous()
            self.sources = _sources_c(None, 0, None, self.d["cov3D"])
        entry = "_aux" if aux else "_ex" if cov else ""
        self.state, image, depth, alpha = _call_forward(self.cs, self.d, self.cap, entry, self.sources)
        state2, image2, depth2, alpha2 = _call_forward(self.cs, self.d, self.cap, entry, self.sources)
        n, overflow = self.state.counters()[:2]
        assert overflow == 0 and n == fw.num_rendered
        HW = self.H * self.W
        self.pads_clean = all(_untouched(t[m:]).all() for t, m in ((image, 3 * HW),) + (((depth, HW), (alpha, HW)) if aux else ()))
        self.maps_left_alone = aux or (_untouched(depth).all() and _untouched(alpha).all())
        fT, nc = self.state.image_aux()
        fT2, nc2 = state2.image_aux()
        self.repeatable = (torch.equal(image.view(torch.int32), image2.view(torch.int32)) and torch.equal(fT.view(torch.int32), fT2.view(torch.int32))
                           and torch.equal(nc, nc2) and (not aux or (torch.equal(depth.view(torch.int32), depth2.view(torch.int32))
                                                                     and torch.equal(alpha.view(torch.int32), alpha2.view(torch.int32)))))
        self.image = image[: 3 * HW].view(3, self.H, self.W).cpu().numpy()
        self.depth = depth[:HW].view(self.H, self.W).cpu().numpy() if aux else None
        self.alpha = alpha[:HW].view(self.H, self.W).cpu().numpy() if aux else None
        self.final_T, self.n_contrib = fT.cpu().numpy(), nc.cpu().numpy()
        self.radii = self.state.radii.cpu().numpy()
        # the lists are the oracle's, bit for bit (tests/test_raster_gpu.py holds that on its own scenes)
        off, pl = self.state.tile_lists()
        self.off, self.pl = off.cpu().numpy().astype(np.int64), pl.cpu().numpy()
        assert np.array_equal(self.radii, fw.radii) and np.array_equal(self.pl, fw.point_list)
        assert np.array_equal(np.diff(self.off), fw.tile_ranges[:, 1] - fw.tile_ranges[:, 0])
        self.ranges = np.stack([self.off[:-1], self.off[1:]], axis=1)
        # the fp32 numbers the kernel itself stored, cast up by the references
        G = self.G = _geom_records(self.state)
        Gf = G.view(np.float32)
        self.geom6 = np.stack([Gf[:, 0], Gf[:, 1], Gf[:, 14], Gf[:, 2], Gf[:, 3], Gf[:, 4]], axis=1)
        self.opac, self.col = Gf[:, 5].copy(), Gf[:, 6:9].copy()
        live = self.radii > 0
        self.opac[~live], self.col[~live], self.geom6[~live] = 1.0, 0.0, 0.0          # (never listed: only kept finite)
        self.lists = (self.geom6, self.opac, self.col, self.ranges, self.pl, self.st)
        self.r64, self.r32, self.border = K.forward_refs(*self.lists, fw.borderline, maps=aux)
        self.forms = ("literal", "poly") if name.startswith("L") else ("poly",)
        self.unsafe = K.unsafe_conic(self.geom6) & live       # Gaussians whose chunks take the literal loops (scene L's needles)

    def e32_of(self, f):
        """The larger error of the float32 runs of the forms this scene's kernels take; f(run) -> error."""
        return max(f(self.r32[form]) for form in self.forms)

    def rows_of_instances(self):
        """Per list position: its row in scratch (goff + row-major place in the rectangle) and whether its alpha box touches its tile."""
        G, gx = self.G, (self.W + 15) // 16
        tile = np.repeat(np.arange(len(self.off) - 1), np.diff(self.off))
        tx, ty = tile % gx, tile // gx
        g = G[self.pl]
        rx0, rx1, ry0 = g[:, 12] & 0xFFFF, g[:, 12] >> 16, g[:, 13] & 0xFFFF
        row = g[:, 11].view(np.int32).astype(np.int64) + (ty - ry0.astype(np.int64)) * (rx1.astype(np.int64) - rx0) + (tx - rx0.astype(np.int64))
        bx0, bx1, by0, by1 = _s16(g[:, 9]), _s16(g[:, 9] >> 16), _s16(g[:, 10]), _s16(g[:, 10] >> 16)
        hit = ~((bx0 > tx * 16 + 15) | (bx1 < tx * 16) | (by0 > ty * 16 + 15) | (by1 < ty * 16))
        return row, hit


@functools.lru_cache(maxsize=None)
def _fwd(name, bg, aux=False, view="viewmatrix", cov=False):
    return _Fwd(name, bg, aux, view, cov)


def _upstream(f, seed, maps=False):
    rng = np.random.default_rng(seed)
    dL = rng.standard_normal((3, f.H, f.W)).astype(np.float32)
    dL[:, f.border] = 0
    if not maps:
        return dL, None, None
    gD, gA = rng.standard_normal((f.H, f.W)).astype(np.float32), rng.standard_normal((f.H, f.W)).astype(np.float32)
    gD[f.border], gA[f.border] = 0, 0
    return dL, gD, gA


def _call_backward(f, flags, dL, gD=None, gA=None, probe=False):
    """gsvc_raster_backward{,_ex,_aux} of the forward `f` with test-owned, NaN-filled scratch and outputs.  Returns (scratch [rows, 16]
    uint32 with the tail rows and pad, the six gradients (seven, "cov3D", when `f` has the covariance source), True when every pad
    is untouched)."""
    from gsvc_amd import rasterizer
    L, p = _lib.lib(), _lib.ptr
    cs = _c_settings(f.s, f.bg, f.view, flags=int(f.s.get("flags", 0)) | flags)
    P, cap, d, st = f.P, f.cap, f.d, f.state
    n_scr = rasterizer.backward_scratch_floats(P, cap)
    assert n_scr == 16 * cap
    scratch = _nan_buf(n_scr)
    sizes = (3, 3, 3, 1, 3, 4)
    grads = [_nan_buf(P * k) for k in sizes]
    dev = lambda a: None if a is None else torch.tensor(a, device="cuda").contiguous()
    dLt, gDt, gAt = dev(dL), dev(gD), dev(gA)
    aux = gD is not None or gA is not None
    ex = f.sources is not None
    assert not (aux and ex)
    dcov = _nan_buf(P * 6) if ex else None
    name = "gsvc_raster_backward" + ("_aux" if aux else "_ex" if ex else "")
    sr = [None, None] if ex else [p(d["scales"]), p(d["rotations"])]
    args = [C.byref(cs), P, cap, p(d["means3D"]), p(d["colors"]), p(d["opacities"])] + sr
    args += ([None] if aux else [C.byref(f.sources)] if ex else []) + [p(st.radii), p(st.geom), p(st.binning), p(st.image_state), p(dLt)]
    args += ([p(gDt), p(gAt)] if aux else []) + [p(g) for g in grads] + ([None, p(dcov)] if aux or ex else [])
    if probe:
        _lib.profile_enable(2)
    try:
        _lib.check(getattr(L, name)(*args, p(scratch), _lib.current_stream(torch.device("cuda"))), name)
        torch.cuda.synchronize()
    finally:
        if probe:
            _lib.profile_enable(0)
    pads = all(_untouched(g[P * k:]).all() for g, k in zip(grads, sizes)) and _untouched(scratch[n_scr:]).all()
    rows = scratch[:n_scr].view(torch.int32).view(cap, 16).cpu().numpy().view(np.uint32)
    out = {k: g[: P * n].view(P, n).cpu().numpy() for k, g, n in zip(("means3D", "means2D", "colors", "opacities", "scales", "rotations"), grads, sizes)}
    if ex:
        pads = pads and _untouched(dcov[P * 6:]).all()
        out["cov3D"] = dcov[: P * 6].view(P, 6).cpu().numpy()
    return rows, out, pads


# ------------------------------------------------------------------------------------------------------------ 1. GeomRec
@pytest.mark.parametrize("name", ["R400", "L300", "B"])
def test_geomrec_fields(name):
    f = _fwd(name, BG)
    G, Gf, fw = f.G, f.G.view(np.float32), f.fw
    live = f.radii > 0
    assert live.sum() > 10
    # u, v, A, B, C, depth: the oracle's geom bit for bit
    for col_g, col_o in ((0, 0), (1, 1), (14, 2), (2, 3), (3, 4), (4, 5)):
        assert np.array_equal(G[live, col_g], fw.geom[live, col_o].view(np.uint32)), col_g
    assert np.array_equal(G[live, 5], f.sc["opacities"].reshape(-1)[live].view(np.uint32))
    assert np.array_equal(G[live, 6:9], f.sc["colors"][live].view(np.uint32))
    # the tile rectangle: every tile the oracle lists the Gaussian in lies inside it, and it has as many tiles as the oracle counts
    rx0, rx1, ry0, ry1 = (G[:, 12] & 0xFFFF).astype(np.int64), (G[:, 12] >> 16).astype(np.int64), (G[:, 13] & 0xFFFF).astype(np.int64), (G[:, 13] >> 16).astype(np.int64)
    n_tiles = (rx1 - rx0) * (ry1 - ry0)
    assert np.array_equal(n_tiles[live], fw.geom[live, 7].astype(np.int64)) and not n_tiles[~live].any()
    gx = (f.W + 15) // 16
    tile = np.repeat(np.arange(len(f.off) - 1), np.diff(f.off))
    tx, ty, ids = tile % gx, tile // gx, f.pl
    assert np.all((tx >= rx0[ids]) & (tx < rx1[ids]) & (ty >= ry0[ids]) & (ty < ry1[ids]))
    # goff: the blocks [goff, goff + tiles) of the live Gaussians are disjoint and fill [0, num_rendered) without a gap
    goff = G[:, 11].view(np.int32).astype(np.int64)
    order = np.argsort(goff[live], kind="stable")
    starts, lens = goff[live][order], n_tiles[live][order]
    assert starts[0] == 0 and np.array_equal(starts[1:], (starts + lens)[:-1]) and starts[-1] + lens[-1] == fw.num_rendered
    row, _ = f.rows_of_instances()
    assert np.array_equal(np.sort(row), np.arange(fw.num_rendered))            # one row per instance, in rectangle order
    # the alpha box is conservative: no pixel of the 3-sigma rectangle outside it reaches a float64 alpha of (1 + 1e-4) / 255
    bx0, bx1, by0, by1 = _s16(G[:, 9]), _s16(G[:, 9] >> 16), _s16(G[:, 10]), _s16(G[:, 10] >> 16)
    g64, o64 = f.geom6.astype(np.float64), f.opac.astype(np.float64)
    outside_pixels = 0
    for i in np.nonzero(live)[0]:
        xs = np.arange(rx0[i] * 16, min(rx1[i] * 16, f.W))
        ys = np.arange(ry0[i] * 16, min(ry1[i] * 16, f.H))
        X, Y = np.meshgrid(xs, ys)
        out = (X < bx0[i]) | (X > bx1[i]) | (Y < by0[i]) | (Y > by1[i])
        dx, dy = g64[i, 0] - X, g64[i, 1] - Y
        power = -0.5 * (g64[i, 3] * dx * dx + g64[i, 5] * dy * dy) - g64[i, 4] * dx * dy
        a = np.where(power <= 0, o64[i] * np.exp(np.minimum(power, 0)), 0.0)
        outside_pixels += int(out.sum())
        assert not np.any(a[out] >= (1 + 1e-4) / 255.0), (i, float(a[out].max()))
    assert outside_pixels > 0


# ------------------------------------------------------------------------------------------------------------ 2. k_blend
FWD_CASES = [("R300", BLACK, False), ("R400", BG, True), ("R600", BG, False), ("L300", BG, True), ("B", BLACK, False)]
FWD_CASES += [(f"S{n}", BLACK if i % 2 else BG, False) for i, n in enumerate(K.STACK_COUNTS)]
FWD_CASES += [(f"S{n}c", BG if i % 2 else BLACK, False) for i, n in enumerate(K.STACK_COUNTS)]


@pytest.mark.parametrize("name,bg,aux", FWD_CASES)
def test_k_blend_against_float64(name, bg, aux):
    f = _fwd(name, bg, aux)
    ok = ~f.border
    share = f.border.mean()
    if os.environ.get("GSVC_PRINT_ERRORS"):
        print(f"RASTER_BORDERLINE {name}: {share:.3e} (cap {K.borderline_cap(name):g})")
    assert share <= K.borderline_cap(name)
    assert f.repeatable and f.pads_clean and f.maps_left_alone
    assert np.array_equal(f.n_contrib[ok], f.r64["n_contrib"][ok])
    ok3 = np.broadcast_to(ok, (3,) + ok.shape)
    r64 = f.r64
    err = lambda got, key, scale, keep: K.rule_error(got, r64[key], scale, keep)
    one = np.ones((f.H, f.W))
    _assert_rule(f"{name} image", err(f.image, "image", r64["image_scale"], ok3),
                 f.e32_of(lambda r: err(r["image"], "image", r64["image_scale"], ok3)), err(f.fw.image, "image", r64["image_scale"], ok3))
    _assert_rule(f"{name} final_T", err(f.final_T, "final_T", one, ok), f.e32_of(lambda r: err(r["final_T"], "final_T", one, ok)),
                 err(f.fw.final_T, "final_T", one, ok))
    if aux:
        _assert_rule(f"{name} depth", err(f.depth, "depth", r64["depth_scale"], ok), f.e32_of(lambda r: err(r["depth"], "depth", r64["depth_scale"], ok)))
        _assert_rule(f"{name} alpha", err(f.alpha, "alpha", one, ok), f.e32_of(lambda r: err(r["alpha"], "alpha", one, ok)))


# ----------------------------------------------------------------------------------------------------- 3. two-view frame
def test_two_view_frame_against_float64():
    """gsvc_raster_forward_pair against 0.5 (ref64(view) + flip_W(ref64(opposite view))), each half from that view's own single-view
    GeomRec and lists; borderline: the union of the two."""
    a, b = _fwd("R300", BG), _fwd("R300", BG, False, "viewmatrix_s")
    _, image, _, _ = _call_forward(a.cs, a.d, 2 * a.cap + 1024, "_pair")
    HW = a.H * a.W
    assert _untouched(image[3 * HW:]).all()
    got = image[: 3 * HW].view(3, a.H, a.W).cpu().numpy()
    pair = lambda x, y: 0.5 * (np.asarray(x, np.float64) + np.asarray(y, np.float64)[..., ::-1])
    ref, scale = pair(a.r64["image"], b.r64["image"]), pair(a.r64["image_scale"], b.r64["image_scale"])
    border = a.border | b.border[:, ::-1]
    assert border.mean() <= K.borderline_cap("R300")
    ok3 = np.broadcast_to(~border, (3, a.H, a.W))
    e32 = K.rule_error(pair(a.r32["poly"]["image"], b.r32["poly"]["image"]), ref, scale, ok3)
    _assert_rule("R300 pair image", K.rule_error(got, ref, scale, ok3), e32, K.rule_error(pair(a.fw.image, b.fw.image), ref, scale, ok3))


# ------------------------------------------------------------------------------------------- 4. k_blend_bwd_tile's rows
CS = K.F_CLAMP_STOP
BWD_CASES = [("R300", BLACK, 0, False, False), ("R400", BG, CS, False, False), ("R600", BG, 0, False, False),
             ("R400", BG, 0, True, False), ("L300", BG, 0, False, False), ("L300", BG, CS, False, True),
             ("B", BLACK, 0, False, False), ("B", BG, CS, False, False), ("S65c", BG, 0, False, False)]
BWD_CASES += [(f"S{n}", BLACK if i % 2 else BG, CS if i % 2 else 0, False, False) for i, n in enumerate(K.STACK_COUNTS)]
BWD_CASES += [(f"S{n}c", BG if i % 2 else BLACK, CS, False, False) for i, n in enumerate(K.STACK_COUNTS)]


def _rows_refs(f, flags, dL, gD, gA, forms):
    st = dict(f.st, flags=int(f.st.get("flags", 0)) | flags)
    args = f.lists[:5] + (st, f.final_T, f.r64["decisions"], dL)
    ref, mags = K.blend_bwd_rows_ref(*args, np.float64, "literal", gD, gA)
    r32 = {form: K.blend_bwd_rows_ref(*args, np.float32, form, gD, gA)[0] for form in forms}
    return ref, mags, r32


@pytest.mark.parametrize("name,bg,flags,aux,probe", BWD_CASES)
def test_k_blend_bwd_tile_rows_against_float64(name, bg, flags, aux, probe):
    """`scratch` read back after the backward: every element of every row on its own sum of absolute terms.  (S129 on the non-zero
    background is the case that found the background's share of dL/dalpha subtracted as a separate term: 1.33e-5 against a bound
    of 8.3e-6; 4.5e-6 since the background starts the behind-colour recurrence)"""
    f = _fwd(name, bg, aux)
    assert f.border.mean() <= K.borderline_cap(name)
    dL, gD, gA = _upstream(f, 11, aux)
    rows, grads, pads = _call_backward(f, flags, dL, gD, gA, probe)
    assert pads
    ns = 10 if aux else 9
    n_inst = f.fw.num_rendered
    row, hit = f.rows_of_instances()
    # rows nobody owns (the tail) and rows of instances whose alpha box misses their tile: still the NaN pattern, all 16 floats
    assert np.all(rows[n_inst:] == NAN_BITS)
    assert np.all(rows[row[~hit]] == NAN_BITS)
    if name == "B":
        assert (~hit).sum() > 0
    # every instance whose box touches its tile: written whole, floats 9 (10) .. 15 are +0
    got = rows[row[hit]]
    assert np.all(got[:, ns:] == 0)
    vals = got[:, :ns].view(np.float32)
    assert np.all(np.isfinite(vals))
    forms = ("literal",) if probe else f.forms
    ref, mags, r32 = _rows_refs(f, flags, dL, gD, gA, forms)
    assert not np.any(mags[~hit])                        # an instance without a row has nothing to say in float64 either
    assert np.abs(ref).max() > 0
    e_k = K.rule_error(vals, ref[hit], mags[hit])        # zero scale (entries behind the last contributor): exact zeros
    e32 = _e32({form: r[hit] for form, r in r32.items()}, ref[hit], mags[hit], f.unsafe[f.pl][hit])
    if name == "S129c":
        assert np.any((mags[hit] == 0).all(axis=1))      # a list that stopped early left such entries
    _assert_rule(f"{name} flags={flags} aux={aux} probe={probe} rows", e_k, e32)


# ----------------------------------------------------------------------------------------------- 5. k_gaussian_bwd alone
@pytest.mark.parametrize("name,bg,aux,cov", [("B", BG, False, False), ("R400", BG, True, False), ("B", BG, False, True)])
def test_k_gaussian_bwd_on_its_own_rows(name, bg, aux, cov):
    """Inputs: the rows k_blend_bwd_tile wrote, read back and cast up; a Gaussian's rows are added in tile order.  cov: the
    covariance source (gsvc_raster_forward_ex / _backward_ex with cov3D, no scales or rotations): the seventh output dL/dcov3D
    under the rule, dL/dscales and dL/drotations exact zeros."""
    f = _fwd(name, bg, aux, "viewmatrix", cov)
    dL, gD, gA = _upstream(f, 12, aux)
    rows, grads, pads = _call_backward(f, 0, dL, gD, gA)
    assert pads
    ns = 10 if aux else 9
    row, hit = f.rows_of_instances()
    # the rows of instances whose alpha box misses their tile were never written: still NaN in THIS call, and there are some
    assert (~hit).any() and np.all(rows[row[~hit]] == NAN_BITS)
    vals = np.zeros((len(row), ns), np.float32)
    vals[hit] = rows[row[hit]][:, :ns].view(np.float32)
    order = np.argsort(row, kind="stable")               # a Gaussian's rows in rectangle (= tile) order
    tot = K.sum_rows_per_gaussian(vals[order], f.pl[order], f.P)
    mag = K.sum_rows_per_gaussian(np.abs(vals[order]), f.pl[order], f.P)
    tot32 = K.sum_rows_per_gaussian(vals[order], f.pl[order], f.P, np.float32)
    inp = dict(means3D=f.sc["means3D"], opacities=f.sc["opacities"], radii=f.radii)
    inp.update(dict(cov3D=f.cov) if cov else dict(scales=f.sc["scales"], rotations=f.sc["rotations"]))
    ref, scale, r32 = (K.gaussian_bwd_ref(tot, inp, f.st, np.float64), K.gaussian_bwd_ref(mag, inp, f.st, np.float64, mag=True),
                       K.gaussian_bwd_ref(tot32, inp, f.st, np.float32))
    dead = (f.radii == 0) | (f.sc["opacities"].reshape(-1) <= 0)
    if name == "B":
        assert dead.sum() >= 3                           # culled by the slab, the screen and opacity <= 0
    for k in K.GRADS + (("cov3D",) if cov else ()):
        assert np.all(np.isfinite(grads[k])), k          # NaN rows are never read
        assert not np.any(grads[k][dead]), k             # exact zeros
        if cov and k in ("scales", "rotations"):
            assert not np.any(grads[k]) and not np.any(ref[k]), k
            continue
        assert np.abs(ref[k]).max() > 0
        _assert_rule(f"{name} aux={aux} cov={cov} k_gaussian_bwd {k}", K.rule_error(grads[k], ref[k], scale[k]),
                     K.rule_error(r32[k], ref[k], scale[k]))


# -------------------------------------------------------------------------------------------- 6. end to end, per Gaussian
@pytest.mark.parametrize("name,probe", [("R300", False), ("R400", False), ("R600", False), ("L300", False), ("L300", True)])
def test_autograd_gradients_per_gaussian_against_the_float64_chain(oracle_lib, name, probe):
    """The assertion `max |got - ref| / max |ref|` cannot make: every element of the six gradients on its own scale.  The worst
    element's scale relative to the tensor's largest is printed."""
    from gsvc_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    f = _fwd(name, BG)
    dL, _, _ = _upstream(f, 13)
    d = {k: torch.tensor(f.sc[k], device="cuda", requires_grad=True) for k in IN}
    means2D = torch.zeros_like(d["means3D"], requires_grad=True)
    s = f.s
    r = GaussianRasterizer(raster_settings=GaussianRasterizationSettings(
        image_height=s["H"], image_width=s["W"], x_min=s["x_min"], y_min=s["y_min"], scale=s["scale"], threshold=s["threshold"],
        bg=torch.tensor(BG, dtype=torch.float32), scale_modifier=s["scale_modifier"], viewmatrix=torch.tensor(s["viewmatrix"]),
        sh_degree=0, campos=torch.tensor([0.0, 0.0, s["z_cam"]]), prefiltered=False, debug=False, flags=s.get("flags", 0),
        low_pass=s.get("low_pass", 0.0)))
    if probe:
        _lib.profile_enable(2)
    try:
        image, _, _ = r(means3D=d["means3D"], means2D=means2D, shs=None, colors_precomp=d["colors"], opacities=d["opacities"],
                        scales=d["scales"], rotations=d["rotations"], cov3D_precomp=None)
        (image * torch.tensor(dL, device="cuda")).sum().backward()
        torch.cuda.synchronize()
    finally:
        if probe:
            _lib.profile_enable(0)
    got = {k: d[k].grad.cpu().numpy() for k in IN}
    got["means2D"] = means2D.grad.cpu().numpy()
    rb = oracle_lib.raster_backward(K.oracle_settings(oracle_lib, f.s, bg=BG), f.sc["means3D"], f.sc["colors"], f.sc["opacities"], f.sc["scales"],
                                    f.sc["rotations"], f.fw, dL)
    args = f.lists
    inp = dict(means3D=f.sc["means3D"], scales=f.sc["scales"], rotations=f.sc["rotations"], opacities=f.sc["opacities"], radii=f.radii)

    def chain(dtype, form, final_T):
        rows, mags = K.blend_bwd_rows_ref(*args, final_T, f.r64["decisions"], dL, dtype, form)
        return (K.gaussian_bwd_ref(K.sum_rows_per_gaussian(rows, f.pl, f.P, dtype), inp, f.st, dtype),
                K.sum_rows_per_gaussian(mags, f.pl, f.P))
    ref, mags = chain(np.float64, "literal", f.r64["final_T"])
    scale = K.gaussian_bwd_ref(mags, inp, f.st, np.float64, mag=True)
    r32 = {form: chain(np.float32, form, f.r32[form]["final_T"])[0] for form in (("literal",) if probe else f.forms)}
    for k in K.GRADS:
        g = got[k].reshape(ref[k].shape)
        e_k = K.rule_error(g, ref[k], scale[k])
        e32 = _e32({form: x[k] for form, x in r32.items()}, ref[k], scale[k], f.unsafe)
        nz = scale[k] > 0
        worst = np.unravel_index(np.argmax(np.where(nz, np.abs(g - ref[k]) / np.where(nz, scale[k], 1.0), 0.0)), g.shape)
        if os.environ.get("GSVC_PRINT_ERRORS"):
            print(f"RASTER_WORST {name} probe={probe} {k}: element {worst}, its scale / the tensor's largest = {scale[k][worst] / scale[k].max():.2e}, "
                  f"smallest scale / largest = {scale[k][nz].min() / scale[k].max():.2e}")
        _assert_rule(f"{name} probe={probe} end-to-end {k}", e_k, e32, K.rule_error(getattr(rb, k).reshape(ref[k].shape), ref[k], scale[k]))
