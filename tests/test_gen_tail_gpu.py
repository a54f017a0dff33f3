"""k_gen_tail_fwd / k_gen_tail_bwd (csrc/generate.hip) through generate._GenTail against the float64 statement of the same five
formulas (tests/_step_kernel_refs.gen_tail_ref), at every rows-per-block packing the backward has (rpb = 256 // K, rows around
multiples of rpb), with zero quaternions, saturated sigmoids, Gaussians exactly on and far outside the bounds placed in the first,
an interior and the last block, and for every subset of outputs the training step differentiates.

Tolerances.  Exact (torch.equal) where an output is one fp32 rounding of its inputs or a selection: neural_opacity, mask, xyz from
world, d_op_raw, d_offset_mask, zeros.  Everything else: e_kernel <= 4 * e32 + 4 * eps32, where e32 is the error of the same tensor
statement evaluated in fp32 on the same inputs, both against float64 and on the same scale.  The kernel and the fp32 statement are two
legitimate fp32 evaluations of one formula (contracted a + b * c, expf / sqrtf / reciprocal a few ulp apart, multiply by 1 / |q|
against divide), each output at most eight roundings deep, so neither is more than a small multiple of the other; a wrong branch,
row or a dropped term is wrong by the size of the term.  Scale: elementwise outputs by the tensor's largest magnitude; the per-row
sums (d_grid_scaling, d_anchor) row by row and component by component by the float64 sum of the absolute values of the row's K terms;
d_scale_rot[3:7] of the zero-quaternion Gaussians (of size 1e12 * g) separately from the rest of d_scale_rot.

Inputs keep float64 and fp32 on the same side of every discontinuity (asserted on the reference before the kernel is looked at): no
|op_raw * offset_mask| in (0, 1e-30), quaternion norms 0 or >= 1e-3, no world component within 1e-4 * max|bound| of a bound except
the constructed on-bound Gaussians.  An input that violates one is redrawn; no element is left out of any comparison.

GSVC_PRINT_ERRORS=1 prints every e_kernel and e32.
"""
import pytest
import torch

from tests._step_kernel_refs import EPS32, PRINT, err, err_each, gen_tail_expanded, gen_tail_ref

pytestmark = pytest.mark.gpu


LO, HI = (-1.5, -1.25, -1.75), (1.5, 1.75, 1.25)          # exact in fp32, different per component
BAND = 1e-4 * max(max(abs(v) for v in LO + HI), 1.0)
KS = (1, 3, 4, 7, 10, 100, 129, 256)
IN_NAMES = ("op_raw", "offset_mask", "grid_offsets", "neural_offset", "scale_rot", "grid_scaling", "anchor")
OUT_NAMES = ("neural_opacity", "scaling", "rot", "world", "xyz")      # the differentiable outputs, in the order of the tuple
ALL = frozenset(OUT_NAMES)
SUBSETS = (ALL, ALL - {"world"}, frozenset({"xyz", "neural_opacity"}), frozenset({"rot"}))


def _rows_for(K):
    rpb = 256 // K
    rows = {1, rpb - 1, rpb, rpb + 1, 5 * rpb + 2} | ({60011} if K in (4, 10) else set())
    return sorted(r for r in rows if r > 0)


CASES = [(K, rows) for K in KS for rows in _rows_for(K)]


def _inputs(K, rows, seed=0):
    """fp32 inputs on the host and the indices of the constructed Gaussians: dict of name -> tensor, dict of kind -> index tensor."""
    g = torch.Generator().manual_seed(1000 * K + rows + seed)
    n, rpb = rows * K, 256 // K if K <= 256 else 1
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = {"op_raw": rn(n), "scale_rot": rn(n, 7), "anchor": rn(rows, 3),
         "grid_offsets": 0.3 * rn(n, 3), "neural_offset": 0.3 * rn(n, 3),
         "grid_scaling": torch.rand(rows, 6, generator=g) + 0.1}
    u = torch.rand(n, generator=g)
    t["offset_mask"] = torch.where(u < 0.25, torch.zeros(n), torch.where(u < 0.75, torch.ones(n), 0.5 + u))
    # constructed Gaussians in the first, an interior and the last block of the backward (a block = rpb anchor rows)
    nb = (rows + rpb - 1) // rpb
    kinds = {"on_bound": [], "outside": [], "zero_quat": [], "saturated": []}
    for b in sorted({0, nb // 2, nb - 1}):
        i0, i1 = b * rpb * K, min(rows, (b + 1) * rpb) * K          # the block's Gaussians
        pick = lambda j: i0 + j if i0 + j < i1 else i0  # noqa: E731
        kinds["on_bound"] += [i0, i1 - 1]
        kinds["outside"] += [i for i in (i0 + 1, i1 - 2) if i0 < i < i1 - 1]
        kinds["zero_quat"] += [pick(2), i1 - 1]
        kinds["saturated"] += [pick(3), i1 - 1]
    kinds = {k: torch.tensor(sorted(set(v)), dtype=torch.int64) for k, v in kinds.items()}
    lo, hi = torch.tensor(LO), torch.tensor(HI)
    for j, i in enumerate(kinds["on_bound"].tolist()):               # offsets zero, anchor on the bound: world == anchor in any precision
        up = torch.tensor([(j + c) % 2 == 1 for c in range(3)])
        t["anchor"][i // K] = torch.where(up, hi, lo)
        t["grid_offsets"][i], t["neural_offset"][i] = 0.0, 0.0
    for i in kinds["outside"].tolist():                               # 5 beyond the anchor, away from the origin: |world| > 5
        a = t["anchor"][i // K]
        t["grid_offsets"][i] = torch.where(a >= 0, 5.0, -5.0) / t["grid_scaling"][i // K, 0:3]
        t["neural_offset"][i] = 0.0
    t["scale_rot"][kinds["zero_quat"], 3:7] = 0.0
    for j, i in enumerate(kinds["saturated"].tolist()):
        t["scale_rot"][i, 0:3] = torch.tensor([100.0, -100.0, 100.0]) * (1 if j % 2 == 0 else -1)
    # redraw the offsets of Gaussians whose float64 world lies inside the band around a bound (before anything is compared)
    free = torch.ones(n, dtype=torch.bool)
    free[kinds["on_bound"]] = False
    for _ in range(20):
        bad = (_near_bound(_world64(t, K)).any(dim=1) & free).nonzero().squeeze(1)
        if bad.numel() == 0:
            break
        t["grid_offsets"][bad], t["neural_offset"][bad] = 0.3 * rn(bad.numel(), 3), 0.3 * rn(bad.numel(), 3)
    return t, kinds


def _world64(t, K):
    d = {k: v.double() for k, v in t.items()}
    return gen_tail_ref(*(d[k] for k in IN_NAMES), K, LO, HI)[4]


def _near_bound(world):
    lo, hi = (torch.tensor(v, dtype=world.dtype, device=world.device) for v in (LO, HI))
    return ((world - lo).abs() <= BAND) | ((world - hi).abs() <= BAND)


def _assert_conditions(t64, ref_out, kinds, K):
    """The input conditions of the module docstring, on the float64 reference."""
    no, _, _, _, world, _ = ref_out
    a = no.abs()
    assert not ((a > 0) & (a < 1e-30)).any()
    nrm = t64["scale_rot"][:, 3:7].norm(dim=1)
    assert ((nrm == 0) | (nrm >= 1e-3)).all()
    assert torch.equal((nrm == 0).nonzero().squeeze(1).cpu(), kinds["zero_quat"])
    near = _near_bound(world).any(dim=1).nonzero().squeeze(1).cpu()
    assert torch.equal(near, kinds["on_bound"]), (near, kinds["on_bound"])
    ob = kinds["on_bound"].to(world.device)
    lo, hi = (torch.tensor(v, dtype=world.dtype, device=world.device) for v in (LO, HI))
    assert ((world[ob] == lo) | (world[ob] == hi)).all()                   # exactly on it, every component
    assert torch.equal(world[ob], t64["anchor"][ob // K])
    out = kinds["outside"].to(world.device)
    assert ((world[out] < lo - 1) | (world[out] > hi + 1)).all()


def _cuda(t, dtype, grad=True, anchor_grad=True):
    return {k: v.to("cuda", dtype).requires_grad_(grad and (anchor_grad or k != "anchor")) for k, v in t.items()}


def _weights(n, seed, scale=1.0):
    g = torch.Generator().manual_seed(77 + seed)
    return {nm: (scale * torch.randn(n, c, generator=g)).to("cuda") for nm, c in zip(OUT_NAMES, (1, 3, 4, 3, 3))}


def _loss(outs, w, use):
    named = dict(zip(OUT_NAMES, (outs[0], outs[2], outs[3], outs[4], outs[5])))
    return sum((named[nm] * w[nm].to(named[nm].dtype)).sum() for nm in OUT_NAMES if nm in use)


def _kernel(t, K, use=None, w=None, anchor_grad=True):
    """Outputs of _GenTail on fp32 device copies of ``t`` and, with ``use``, the gradients of sum(out * w) over the used outputs."""
    from gsvc_amd.generate import _GenTail
    x = _cuda(t, torch.float32, grad=use is not None, anchor_grad=anchor_grad)
    outs = _GenTail.apply(*(x[k] for k in IN_NAMES), K, LO, HI)
    if use is None:
        return outs, None
    names = [k for k in IN_NAMES if x[k].requires_grad]
    grads = torch.autograd.grad(_loss(outs, w, use), [x[k] for k in names], allow_unused=True)
    assert all(g is not None for g in grads)           # the function returns a tensor for every input, zeros for an unused path
    return outs, dict(zip(names, grads))


def _statement(t, K, dtype, use, w):
    """gen_tail_ref in ``dtype`` on the device: outputs, gradients (zeros where the loss does not reach an input) and, per (row,
    component) of d_grid_scaling / d_anchor, the sum of the absolute values of the K terms the gradient adds up."""
    x = _cuda(t, dtype)
    outs = gen_tail_ref(*(x[k] for k in IN_NAMES), K, LO, HI)
    grads = torch.autograd.grad(_loss(outs, w, use), [x[k] for k in IN_NAMES], allow_unused=True)
    grads = {k: g if g is not None else torch.zeros_like(x[k]) for k, g in zip(IN_NAMES, grads)}
    rows = x["grid_scaling"].shape[0]
    gs_rep = x["grid_scaling"].detach().repeat_interleave(K, dim=0).requires_grad_(True)
    an_rep = x["anchor"].detach().repeat_interleave(K, dim=0).requires_grad_(True)
    outs_e = gen_tail_expanded(*(x[k].detach() for k in IN_NAMES[:5]), gs_rep, an_rep, LO, HI)
    loss_e = _loss(outs_e, w, use)
    terms = torch.autograd.grad(loss_e, [gs_rep, an_rep], allow_unused=True) if loss_e.requires_grad else (None, None)
    terms = [tm if tm is not None else torch.zeros_like(l) for tm, l in zip(terms, (gs_rep, an_rep))]
    abs_sums = {"grid_scaling": terms[0].abs().view(rows, K, 6).sum(dim=1), "anchor": terms[1].abs().view(rows, K, 3).sum(dim=1)}
    return x, outs, grads, abs_sums


def _bound(tag, name, e_kernel, e32):
    if PRINT:
        print(f"GENTAIL_ERR {tag} {name}: kernel {e_kernel:.3e} fp32 statement {e32:.3e}")
    assert e_kernel <= 4 * e32 + 4 * EPS32, (tag, name, e_kernel, e32)


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _elementwise(tag, name, got, s32, ref):
    scale = _maxabs(ref)
    if scale == 0.0:
        assert not got.any(), (tag, name)               # nothing reaches it: zeros, not stale memory
        return
    _bound(tag, name, err(got, ref, scale), err(s32, ref, scale))


@pytest.mark.parametrize("K,rows", CASES)
def test_gen_tail_forward(K, rows):
    """measured on the MI355X, largest over all K and rows, in units of eps32 (kernel / fp32 statement): scaling 1.09 / 1.09,
    rot 1.39 / 1.21, world 0.33 / 0.62."""
    t, kinds = _inputs(K, rows)
    n, tag = rows * K, f"fwd K={K} rows={rows}"
    assert (t["offset_mask"] == 0).any() or n < 8
    assert ((t["op_raw"] < 0).any() and (t["op_raw"] > 0).any()) or n < 8
    w = _weights(n, 0)
    x64, ref, _, _ = _statement(t, K, torch.float64, ALL, w)
    _assert_conditions({k: v.detach() for k, v in x64.items()}, ref, kinds, K)
    x32, s32, _, _ = _statement(t, K, torch.float32, ALL, w)
    (no, mask, scaling, rot, world, xyz), _ = _kernel(t, K)
    assert no.shape == (n, 1) and mask.shape == (n,) and mask.dtype == torch.bool
    assert scaling.shape == (n, 3) and rot.shape == (n, 4) and world.shape == (n, 3) and xyz.shape == (n, 3)
    prod = (x32["op_raw"].detach() * x32["offset_mask"].detach()).view(n, 1)
    assert torch.equal(no, prod) and torch.equal(no, ref[0].float())          # the float64 product is exact: rounded once
    assert torch.equal(mask, (no > 0).view(-1)) and torch.equal(mask, ref[1])
    lo, hi = torch.tensor(LO, device="cuda"), torch.tensor(HI, device="cuda")
    assert torch.equal(xyz, torch.clamp(world, lo, hi))                          # a selection of the kernel's own world
    for name, got, a, b in (("scaling", scaling, s32[2], ref[2]), ("rot", rot, s32[3], ref[3]), ("world", world, s32[4], ref[4])):
        _elementwise(tag, name, got, a.detach(), b.detach())
    zq, ob = kinds["zero_quat"].to("cuda"), kinds["on_bound"].to("cuda")
    assert not rot[zq].any()                                                     # exact zeros
    assert torch.equal(world[ob].double(), ref[4][ob]) and torch.equal(xyz[ob], world[ob])
    sat = kinds["saturated"].to("cuda")
    assert torch.isfinite(scaling).all() and torch.isfinite(scaling[sat]).all()


def test_gen_tail_forward_no_rows():
    t, _ = _inputs(10, 1)
    t = {k: v[:0] for k, v in t.items()}
    outs, _ = _kernel(t, 10)
    assert [tuple(o.shape) for o in outs] == [(0, 1), (0,), (0, 3), (0, 4), (0, 3), (0, 3)]


def _compare_backward(tag, t, K, kinds, use, w, got):
    x64, ref_out, ref, abs_sums = _statement(t, K, torch.float64, use, w)
    _, _, s32, _ = _statement(t, K, torch.float32, use, w)
    n = t["op_raw"].shape[0]
    assert torch.equal(got["grid_offsets"], got["neural_offset"]) and torch.equal(ref["grid_offsets"], ref["neural_offset"])
    # one rounding each
    g_no = w["neural_opacity"].view(-1) if "neural_opacity" in use else torch.zeros(n, device="cuda")
    assert torch.equal(got["op_raw"], g_no * x64["offset_mask"].detach().float())
    assert torch.equal(got["offset_mask"], g_no * x64["op_raw"].detach().float())
    assert err(got["op_raw"], ref["op_raw"], max(_maxabs(ref["op_raw"]), 1.0)) <= EPS32
    assert err(got["offset_mask"], ref["offset_mask"], max(_maxabs(ref["offset_mask"]), 1.0)) <= EPS32
    _elementwise(tag, "d_offsets", got["grid_offsets"], s32["grid_offsets"], ref["grid_offsets"])
    # d_scale_rot: the zero-quaternion Gaussians' [3:7] (1e12 * g) on their own scale, all the rest on the rest's
    zq = torch.zeros(n, 7, dtype=torch.bool, device="cuda")
    zq[kinds["zero_quat"].to("cuda"), 3:7] = True
    d_sr, r_sr, s_sr = got["scale_rot"], ref["scale_rot"], s32["scale_rot"]
    assert torch.isfinite(d_sr).all()
    _elementwise(tag, "d_scale_rot[zero quaternions, 3:7]", d_sr[zq], s_sr[zq], r_sr[zq])
    _elementwise(tag, "d_scale_rot[rest]", d_sr[~zq], s_sr[~zq], r_sr[~zq])
    if "rot" in use:
        g_rot = w["rot"][kinds["zero_quat"].to("cuda")]
        assert err(d_sr[zq].view(-1, 4), g_rot.double() * 1e12, 1e12 * _maxabs(g_rot)) <= 2 * EPS32
    # the row sums, every row on its own scale
    for name in ("grid_scaling", "anchor"):
        if name not in got:
            continue
        q_kernel, q32 = err_each(got[name], ref[name], abs_sums[name]), err_each(s32[name], ref[name], abs_sums[name])
        _bound(tag, f"d_{name}", float(q_kernel.max()), float(q32.max()))
        # ... and against the fp32 statement's error of the same row: where that one is large by construction (K = 1 and the
        # sigmoid saturated at -100: float64 keeps 3.7e-44, fp32 has 0, an error of 1.0 of that row's scale) it must not widen
        # the bound of the other rows
        assert bool((q_kernel <= 4 * q32 + 4 * EPS32).all()), (tag, name)
    # the gate of g_xyz, spelled out: on the bound it arrives (one product, bit-equal when it is the only term), outside it does not
    if "xyz" in use and "world" not in use:
        gs = x64["grid_scaling"].detach().float().repeat_interleave(K, dim=0)[:, 0:3]
        ob, out = kinds["on_bound"].to("cuda"), kinds["outside"].to("cuda")
        assert torch.equal(got["grid_offsets"][ob], w["xyz"][ob] * gs[ob])
        assert not got["grid_offsets"][out].any()
    if "world" in use and kinds["outside"].numel():
        out = kinds["outside"].to("cuda")
        gs = x64["grid_scaling"].detach().float().repeat_interleave(K, dim=0)[:, 0:3]
        assert torch.equal(got["grid_offsets"][out], w["world"][out] * gs[out])    # world's own gradient still arrives
    return ref_out


@pytest.mark.parametrize("K,rows", CASES)
def test_gen_tail_backward(K, rows):
    """All seven input gradients for every subset of outputs the step uses, each right after a backward over all five outputs with
    weights of size 1e6 (a read of a recycled buffer shows up as a wrong value); the anchor without a gradient; two calls bit-equal.

    measured on the MI355X, largest over all K, rows and subsets, in units of eps32 = 1.19e-7 (kernel / fp32 statement):
    d_offsets 0.87 / 0.87, d_scale_rot (rest) 2.75 / 2.10, d_scale_rot (zero quaternions) 0.36 / 0.36, d_grid_scaling 2.20 / 1.74,
    d_anchor 1.77 / 1.32.  At K = 1 a Gaussian saturated at -100 is alone in its row and float64 keeps sigmoid = 3.7e-44 where fp32
    has 0: both errors are 1.0 of that row's (1e-44-sized) scale there, in d_grid_scaling[3:6] and, at rows = 1, in d_scale_rot."""
    t, kinds = _inputs(K, rows)
    n = rows * K
    w = _weights(n, 1)
    big = _weights(n, 2, scale=1e6)
    x64, ref_out, _, _ = _statement(t, K, torch.float64, ALL, w)
    _assert_conditions({k: v.detach() for k, v in x64.items()}, ref_out, kinds, K)
    if n >= 1000:
        outside = ((ref_out[4] < torch.tensor(LO, device="cuda")) | (ref_out[4] > torch.tensor(HI, device="cuda"))).any(dim=1)
        assert 0.1 < float(outside.double().mean()) < 0.9           # both sides of the gate well populated
    first = None
    for use in SUBSETS:
        _kernel(t, K, ALL, big)
        outs, got = _kernel(t, K, use, w)
        _compare_backward(f"bwd K={K} rows={rows} use={'+'.join(nm for nm in OUT_NAMES if nm in use)}", t, K, kinds, use, w, got)
        if use == ALL:
            first = (outs, got)
    # deterministic: a second call on the same input, bit for bit
    outs2, got2 = _kernel(t, K, ALL, w)
    assert all(torch.equal(a, b) for a, b in zip(first[0], outs2))
    assert all(torch.equal(first[1][k], got2[k]) for k in IN_NAMES)
    # the anchor without a gradient (d_anchor is NULL in the kernel): the other six unchanged
    _kernel(t, K, ALL, big)
    _, got3 = _kernel(t, K, ALL, w, anchor_grad=False)
    assert sorted(got3) == sorted(k for k in IN_NAMES if k != "anchor")
    assert all(torch.equal(first[1][k], got3[k]) for k in got3)


@pytest.mark.parametrize("kind", ["column_slice", "expanded"])
def test_gen_tail_anchor_view_gets_its_gradient(kind):
    """An anchor that reaches the function as a non-contiguous view (the wrapper copies it) still receives d_anchor."""
    from gsvc_amd.generate import _GenTail
    K, rows = 10, 77
    t, kinds = _inputs(K, rows)
    if kind == "expanded":       # one anchor for all rows, inside the bounds (the constructed on-bound Gaussians are gone with theirs)
        t["anchor"] = torch.tensor([[0.25, -0.25, 0.125]]).repeat(rows, 1)
    w = _weights(rows * K, 3)
    x = _cuda(t, torch.float32)
    if kind == "column_slice":
        base = torch.cat([x["anchor"].detach(), torch.ones(rows, 2, device="cuda")], dim=1).requires_grad_(True)
        anchor = base[:, 0:3]
    else:
        base = x["anchor"].detach()[:1].clone().requires_grad_(True)
        anchor = base.expand(rows, 3)
    assert not anchor.is_contiguous() and anchor.requires_grad
    outs = _GenTail.apply(*(x[k] for k in IN_NAMES[:6]), anchor, K, LO, HI)
    (g_base,) = torch.autograd.grad(_loss(outs, w, ALL), [base], allow_unused=True)
    assert g_base is not None, "the anchor view received no gradient"
    _, ref_out, ref, abs_sums = _statement(t, K, torch.float64, ALL, w)
    if kind == "expanded":
        assert not _near_bound(ref_out[4]).any()
    _, _, s32, _ = _statement(t, K, torch.float32, ALL, w)
    if kind == "column_slice":
        assert not g_base[:, 3:].any()
        _bound(kind, "d_anchor", err(g_base[:, 0:3], ref["anchor"], abs_sums["anchor"]), err(s32["anchor"], ref["anchor"], abs_sums["anchor"]))
    else:       # the expand's backward adds the rows' gradients up: compared on the sum of all terms' magnitudes
        scale = abs_sums["anchor"].sum(dim=0, keepdim=True)
        _bound(kind, "d_anchor", err(g_base, ref["anchor"].sum(dim=0, keepdim=True), scale),
               err(s32["anchor"].sum(dim=0, keepdim=True), ref["anchor"].sum(dim=0, keepdim=True), scale))


def test_gen_tail_K_above_256():
    """The forward has no limit on K; the backward's block holds whole rows of at most 256 Gaussians and refuses more with the
    library's own error, leaving the device usable."""
    from gsvc_amd import _lib
    K, rows = 257, 3
    t, kinds = _inputs(K, rows)
    w = _weights(rows * K, 4)
    _, ref, _, _ = _statement(t, K, torch.float64, ALL, w)
    _, s32, _, _ = _statement(t, K, torch.float32, ALL, w)
    (no, mask, scaling, rot, world, xyz), _ = _kernel(t, K)
    assert torch.equal(no, ref[0].float()) and torch.equal(mask, ref[1])
    for name, got, a, b in (("scaling", scaling, s32[2], ref[2]), ("rot", rot, s32[3], ref[3]), ("world", world, s32[4], ref[4])):
        _elementwise("fwd K=257", name, got, a.detach(), b.detach())
    with pytest.raises(_lib.GsvcError, match="gen_tail_backward: K > 256"):
        _kernel(t, K, ALL, w)
    torch.cuda.synchronize()
    t2, _ = _inputs(4, 5)
    outs, got = _kernel(t2, 4, ALL, _weights(20, 4))
    torch.cuda.synchronize()
    assert all(torch.isfinite(g).all() for g in got.values())
