"""Plain tensor statements of the second half of csrc/rate.hip (the sampled rate of a fitting step and its normalisation, the
parameter means, the densification statistics) and of csrc/quant.hip (the STE quantiser, the counted STE_binary of the hash tables
and the tables' bit term), written from the header comments of include/gsvc_hip.h and the kernels' own comments.  Called with
float64 tensors they are the references of tests/test_rate_quant_kernels_gpu.py; called with float32 tensors they are "the fp32
tensor statement" those tests calibrate against.  tests/test_rate_quant_kernel_refs_cpu.py pins them, and the GPU file's input
builders (also kept here, so that both files see the same cases), without a GPU.  Nothing here imports the package under test.
"""
import numpy as np
import torch

from tests._loss_kernel_refs import CLAMP_STEPS, EPS32, LOW_BOUND, PRINT, err, err_each, rate_bits_ref, ulp_distance  # noqa: F401

P_MIN32, P_MAX32 = float(np.float32(1e-6)), float(np.float32(1.0) - np.float32(1e-6))      # k_table_bits' clamp constants, as fp32


# ------------------------------------------------------------------------------------------------------------ sampled rate
def render_of(rows, bounds):
    """Render of each row for row offsets bounds[0 .. R]: the number of j in 1 .. R - 1 with row >= bounds[j] (a row at or past the
    last bound belongs to the last render, a row before the first to render 0; empty renders own no row)."""
    R = len(bounds) - 1
    inner = torch.tensor([int(b) for b in bounds[1:R]], dtype=torch.long, device=rows.device)
    return torch.bucketize(rows, inner, right=True)


def rate_sample_bounds(Qg, sel, x_mean_g, bounds):
    """(lo, hi, qm [R], count [R]) of one group: qm[r] = sum of Q over the selected rows of render r / max(count, 1);
    lo / hi [n_sel] = x_mean -+ 15000 qm of the row's render.  Constants: nothing is differentiated through them."""
    R = len(bounds) - 1
    r = render_of(sel, bounds)
    q = Qg.detach().reshape(-1)[sel]
    cnt = torch.zeros(R, dtype=q.dtype, device=q.device).index_add_(0, r, torch.ones_like(q))
    qm = torch.zeros(R, dtype=q.dtype, device=q.device).index_add_(0, r, q) / cnt.clamp_min(1)
    xm = x_mean_g.detach().to(q.dtype)
    return xm - CLAMP_STEPS * qm[r], xm + CLAMP_STEPS * qm[r], qm, cnt


def rate_sample_ref(x, mean, scale, Q, mask, sel, sel_ctx, x_mean, bounds, K, with_raw=False):
    """S [R, 3]: for group g in (feature, scaling, offsets) the bits of the selected rows summed per render.  x[g] [rows, C_g] and
    Q[g] [rows] are read at row sel[i], mean[g] / scale[g] [ctx rows, C_g] at row sel_ctx[i] (None: sel[i]); x is clamped to
    x_mean[g] -+ 15000 (mean of Q[g] over the render's selected rows) and priced by rate_bits_ref; the offsets group is weighted by
    mask[row, col // 3] (None: 1).  Differentiable in x, mean, scale, Q and mask: autograd gives dense gradients with zeros at rows
    that were not selected."""
    R = len(bounds) - 1
    dt, dev = x[0].dtype, x[0].device
    ctx = sel if sel_ctx is None else sel_ctx
    r = render_of(sel, bounds)
    cols, raws = [], []
    for g in range(3):
        lo, hi, _, _ = rate_sample_bounds(Q[g], sel, x_mean[g], bounds)
        bits, raw = rate_bits_ref(x[g][sel], mean[g][ctx], scale[g][ctx], Q[g].reshape(-1)[sel], lo, hi)
        if g == 2 and mask is not None:
            bits = bits * mask.reshape(mask.shape[0], K)[sel].repeat_interleave(3, dim=1)
        cols.append(torch.zeros(R, dtype=dt, device=dev).index_add(0, r, bits.sum(1)))
        raws.append(raw.detach())
    S = torch.stack(cols, dim=1)
    return (S, raws) if with_raw else S


def rate_sample_loop(x, mean, scale, Q, mask, sel, sel_ctx, x_mean, bounds, K):
    """The same sums by a Python loop over rows and columns with math.erf (lists of floats in, a list of lists out): the
    independent statement tests/test_rate_quant_kernel_refs_cpu.py holds rate_sample_ref against."""
    import math
    R = len(bounds) - 1

    def render(row):
        r = 0
        while r + 1 < R and row >= bounds[r + 1]:
            r += 1
        return r

    S = [[0.0] * 3 for _ in range(R)]
    for g in range(3):
        tot, cnt = [0.0] * R, [0] * R
        for s in sel:
            tot[render(s)] += Q[g][s]
            cnt[render(s)] += 1
        for i, s in enumerate(sel):
            e = s if sel_ctx is None else sel_ctx[i]
            r = render(s)
            qm = tot[r] / max(cnt[r], 1)
            lo, hi = x_mean[g] - 15000.0 * qm, x_mean[g] + 15000.0 * qm
            for c in range(len(x[g][s])):
                xc = min(max(x[g][s][c], lo), hi)
                cdf = lambda v: 0.5 * (1.0 + math.erf((v - mean[g][e][c]) / scale[g][e][c] / math.sqrt(2.0)))  # noqa: E731
                lik = max(cdf(xc + 0.5 * Q[g][s]) - cdf(xc - 0.5 * Q[g][s]), 2.0 ** -16)
                w = mask[s][c // 3] if (g == 2 and mask is not None) else 1.0
                S[r][g] += -math.log2(lik) * w
    return S


# ------------------------------------------------------------------------------------------------------------ normalisation
def rate_normalise_ref(S, offset_masks, sel, bounds, dims):
    """(out [R, 4], sum): out[r] = (all, features, scalings, offsets) bits per coded parameter = S / (n_sel_r dims) x keep rate,
    keep rate = rows of render r whose offset masks sum to more than 0 / max(rows of render r, 1), n_sel_r = entries of the sorted
    list sel inside the render; all = (S0 + S1 + S2) / (n_sel_r (d0 + d1 + d2)); sum = sum_r out[r, 0].  A render without sampled
    rows divides by zero, as the expression it stands for does."""
    dt, dev = S.dtype, S.device
    R = len(bounds) - 1
    rows = int(bounds[-1])
    live = offset_masks.reshape(rows, -1).sum(dim=1) > 0
    bt = torch.tensor([int(b) for b in bounds], dtype=torch.long, device=dev)
    cnt = (bt[1:] - bt[:-1]).to(dt)
    kr = torch.stack([live[int(bounds[r]):int(bounds[r + 1])].sum() for r in range(R)]).to(dt) / cnt.clamp_min(1)
    edges = torch.searchsorted(sel, bt)
    N = (edges[1:] - edges[:-1]).to(dt).unsqueeze(1) * torch.tensor([float(d) for d in dims], dtype=dt, device=dev)
    per = S / N * kr.unsqueeze(1)
    tot = ((S[:, 0] + S[:, 1]) + S[:, 2]) / ((N[:, 0] + N[:, 1]) + N[:, 2]) * kr
    return torch.cat([tot.unsqueeze(1), per], dim=1), tot.sum()


def rate_normalise_coef(S, offset_masks, sel, bounds, dims):
    """coef [R, 4] = d out[r, i] / d (the S it divides).  out is linear in S, so the derivative is out at a unit S: column 0 and 1 at
    S = (1, 0, 0), column 2 at (0, 1, 0), column 3 at (0, 0, 1) (autograd would give the same on a sampled render, and nan for every
    entry of an unsampled one: a zero upstream gradient times an infinite factor)."""
    cols = []
    for g in range(3):
        unit = torch.zeros_like(S.detach())
        unit[:, g] = 1
        out, _ = rate_normalise_ref(unit, offset_masks, sel, bounds, dims)
        cols += [out[:, 0], out[:, 1]] if g == 0 else [out[:, 1 + g]]
    return torch.stack(cols, dim=1)


# ------------------------------------------------------------------------------------------------------------ means, statistics
def param_means_ref(feat, scaling, scaling_exp, offset):
    """(means [3], mean absolute terms [3]) of (feat, exp(scaling) if scaling_exp else scaling, offset) over all their elements; an
    empty tensor gives 0 (its sum over max(n, 1))."""
    vals, scales = [], []
    for k, t in enumerate((feat, scaling, offset)):
        v = t.reshape(-1)
        if k == 1 and scaling_exp:
            v = v.exp()
        vals.append(v.sum() / max(v.numel(), 1))
        scales.append(v.abs().sum() / max(v.numel(), 1))
    return torch.stack(vals), torch.stack(scales)


def training_statis_ref(vis, opacity, seen, grad, K, accs):
    """The four accumulators after a call, in the dtype of ``accs`` = (opacity_accum [A], anchor_denom [A], grad_accum [A K],
    denom [A K]): row i of the renders is anchor vis[i] with K Gaussians; opacity_accum += sum_k max(opacity, 0), anchor_denom += 1,
    and where seen: grad_accum[a K + k] += |grad[i K + k, 0:2]|, denom[a K + k] += 1."""
    dt = accs[0].dtype
    rows = vis.shape[0]
    A = accs[0].numel()
    out = [a.detach().clone().reshape(-1) for a in accs]
    o = opacity.to(dt).reshape(rows, K).clamp_min(0)
    out[0].index_add_(0, vis, o.sum(dim=1))
    out[1].index_add_(0, vis, torch.ones(rows, dtype=dt, device=vis.device))
    w = seen.reshape(rows, K).to(dt)
    g = grad.to(dt).reshape(rows * K, -1)[:, :2]
    norm = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]).sqrt().reshape(rows, K)
    out[2] = out[2].reshape(A, K).index_add_(0, vis, norm * w).reshape(-1)
    out[3] = out[3].reshape(A, K).index_add_(0, vis, w).reshape(-1)
    return out


# ------------------------------------------------------------------------------------------------------------ STE quantiser
def ste_bounds_ref(q, x_mean, offs):
    """(bounds [R, 2], raw [R, 2]): raw = x_mean / (mean of q over the render's rows, or the number q) -+ 15000, bounds = trunc(raw),
    in the dtype of x_mean.  An empty render has no mean: nan."""
    dt, dev = x_mean.dtype, x_mean.device
    R = len(offs) - 1
    raw = torch.full((R, 2), float("nan"), dtype=dt, device=dev)
    for r, (lo, hi) in enumerate(zip(offs[:-1], offs[1:])):
        if torch.is_tensor(q) and q.dim() > 0:
            if hi <= lo:
                continue
            qm = q[lo:hi].to(dt).sum() / (hi - lo)
        else:
            qm = torch.as_tensor(q, dtype=dt, device=dev)
        c = x_mean.reshape(()) / qm
        raw[r, 0], raw[r, 1] = c - CLAMP_STEPS, c + CLAMP_STEPS
    return torch.trunc(raw), raw


def quant_slab_sums_ref(x, q, offs):
    """k_quant_sums' partial sums as its comment lays them out: part[r, b] = (sum of x over all columns, sum of q) of rows
    [offs[r] + 64 b, min(offs[r + 1], offs[r] + 64 b + 64)) for b < nbx = ceil(longest render / 64) (at least 1), zeros where a render
    has no such rows; also returns the sums of |x| and |q| (the scales).  [R, nbx, 2] each, in the dtype of x."""
    R = len(offs) - 1
    nbx = max((max(max(b - a for a, b in zip(offs[:-1], offs[1:])), 1) + 63) // 64, 1)
    part = torch.zeros(R, nbx, 2, dtype=x.dtype, device=x.device)
    mag = torch.zeros_like(part)
    for r, (a, e) in enumerate(zip(offs[:-1], offs[1:])):
        for b in range(nbx):
            lo, hi = a + 64 * b, min(e, a + 64 * b + 64)
            if lo < hi:
                part[r, b, 0], part[r, b, 1] = x[lo:hi].sum(), q[lo:hi].sum()
                mag[r, b, 0], mag[r, b, 1] = x[lo:hi].abs().sum(), q[lo:hi].abs().sum()
    return part, mag


def ste_bounds_scalar_f32(q_scalar, x_mean):
    """The two bounds for one scalar step, in fp32 operation by operation: truncf(x_mean / q -+ 15000)."""
    c = np.float32(x_mean) / np.float32(q_scalar)
    return np.trunc(np.float32(c - np.float32(15000.0))), np.trunc(np.float32(c + np.float32(15000.0)))


def ste_fwd_f32(x, Q, bounds, offs):
    """k_ste_fwd in numpy float32, one correctly rounded operation at a time: x1 = min(max(x / Q, lo_r), hi_r) * Q,
    y = x1 + (rint(x1 / Q) * Q - x1); rint rounds ties to even.  x [rows, C] float32, Q [rows] float32 or a number,
    bounds [R, 2] float32.  This is the exact expectation (a float64 run would round another integer next to a tie)."""
    x = np.asarray(x, dtype=np.float32)
    rows = x.shape[0]
    q = np.broadcast_to(np.asarray(Q, dtype=np.float32).reshape(-1, 1), (rows, 1)) if np.ndim(Q) else np.full((rows, 1), Q, np.float32)
    b = np.asarray(bounds, dtype=np.float32).reshape(-1, 2)
    lo, hi = np.empty((rows, 1), np.float32), np.empty((rows, 1), np.float32)
    for r, (a, e) in enumerate(zip(offs[:-1], offs[1:])):
        lo[a:e], hi[a:e] = b[r, 0], b[r, 1]
    v = x / q
    t = np.minimum(np.maximum(v, lo), hi)
    x1 = t * q
    d = x1 / q
    rq = np.rint(d) * q
    diff = rq - x1
    y = x1 + diff
    assert y.dtype == np.float32
    return y


# ------------------------------------------------------------------------------------------------------------ STE binary, table bits
def ste_binary_ref(x):
    """(y, count): y = +1 where x >= 0 (so +0.0 and -0.0 give +1, NaN gives -1), else -1; count = number of +1 entries."""
    pos = x >= 0
    return torch.where(pos, torch.ones_like(x), -torch.ones_like(x)), int(pos.sum())


def ste_binary_bwd_ref(x, g, count_grad):
    """grad x = (g + count_grad / 2) where |x| <= 1, else 0 (NaN: 0); g None = zeros."""
    g = torch.zeros_like(x) if g is None else g
    return torch.where(x.abs() <= 1, g + 0.5 * count_grad, torch.zeros_like(x))


def table_bits_ref(counts, total):
    """(bits, d bits / d ones) in float64 from the tables' counts of +1 entries: p = clamp(ones / total, 1e-6f, 1 - 1e-6f) with the
    two constants the fp32 values cast up; bits = ones (-log2 p) + (total - ones) (-log2 (1 - p)) + 32; the gradient is stated as
    log2((1 - p) / p)."""
    ones = counts.double().sum()
    total = float(total)
    p = torch.clamp(ones / total, min=P_MIN32, max=P_MAX32)
    return ones * (-torch.log2(p)) + (total - ones) * (-torch.log2(1 - p)) + 32, torch.log2((1 - p) / p)


def table_bits_f32(counts, total):
    """The same statement in fp32 tensors on the device of ``counts``.  The counts are integers and stay integers until the
    formula: ones = their sum, zeros = total - ones, each rounded to fp32 once (as is total under the division); everything else
    in fp32."""
    n1 = int(counts.double().sum())
    f = lambda v: torch.tensor(float(v), dtype=torch.float32, device=counts.device)  # noqa: E731
    ones, zeros = f(n1), f(int(total) - n1)
    p = torch.clamp(ones / f(total), min=1e-6, max=1 - 1e-6)
    return ones * (-torch.log2(p)) + zeros * (-torch.log2(1 - p)) + 32, torch.log2((1 - p) / p)


# =================================================================================================================================
# Input builders of tests/test_rate_quant_kernels_gpu.py (CPU tensors; the GPU file moves them over).  Their preconditions are
# asserted for every case by tests/test_rate_quant_kernel_refs_cpu.py with the references above.
# =================================================================================================================================
RS_COLS = {"wide": (50, 6, 10), "one": (1, 1, 1), "c65": (65, 6, 1), "c130": (130, 64, 22)}
# (id, n_sel, column set, rows per render (None: one render of about 2.5 n_sel rows), sel_ctx mode, mask, special)
#   sel_ctx: None, "perm" (distinct context rows), "repeat" (drawn from n_sel / 8 + 1 rows), "three" (all rows share 3 context rows)
#   special: None, "clamp" (the scaling group's step is small: 5-10 % of its elements clamped on each side), "low" (a few per cent
#   of the elements below the likelihood floor), "unsampled" (render 1 has rows but none selected)
RS_CASES = [
    ("n0", 0, "wide", [40, 0, 60], None, True, None),
    ("n1", 1, "wide", None, None, True, None),
    ("n5-wide", 5, "wide", [0, 7, 0, 6, 0], "perm", True, None),
    ("n5-one", 5, "one", None, None, False, None),
    ("n5-c65", 5, "c65", [4, 9], "repeat", True, None),
    ("n5-c130", 5, "c130", None, "three", True, None),
    ("n4096", 4096, "one", None, "repeat", True, None),
    ("n4100-wide", 4100, "wide", [3000, 2500, 0, 4750], "repeat", True, None),
    ("n4100-one", 4100, "one", [5000, 5250], None, True, None),
    ("n4100-c65", 4100, "c65", None, "three", False, None),
    ("n4100-c130", 4100, "c130", [0, 5000, 5250], "perm", True, None),
    ("n4100-R16", 4100, "wide", [0, 700, 650, 1, 800, 0, 640, 700, 660, 2, 690, 700, 710, 0, 3000, 0], "repeat", True, "unsampled"),
    ("n4100-clamp", 4100, "wide", [5000, 5250], None, True, "clamp"),
    ("n4100-low", 4100, "wide", [5000, 5250], "repeat", True, "low"),
    ("n9001", 9001, "c65", [11000, 11500], "repeat", True, None),
    ("n16390-clamp", 16390, "wide", [20000, 0, 20975], None, False, "clamp"),      # the clamped values show the statistics' second trip
]


def rate_sample_case(case):
    """The inputs of one sampled-rate case as a dict of CPU tensors (fp32) and lists.  Built so that no element sits near a decision:
    x = mean + z scale at the selected rows with |z| <= 3 (and a step of at least 0.025 scale: likelihood >= 1e-4), or, in the "low"
    case, with the nearer edge of the bin 6.5 .. 8 scale away (likelihood < 1e-10, fp32 erf saturates); clamp ranges hundreds of
    scales wide except for the scaling group of the "clamp" case, where x is drawn 20 wide around x_mean against a half-width of
    about 30, nothing within 0.1 of either bound, and the mean is placed within 3 scale of the CLAMPED value."""
    cid, n_sel, colset, per_render, ctx_mode, with_mask, special = case
    gen = torch.Generator().manual_seed(1000 + sum(ord(c) for c in cid))
    Cf, Cs, K = RS_COLS[colset]
    C = (Cf, Cs, 3 * K)
    rows = sum(per_render) if per_render is not None else max(int(2.5 * n_sel), 3)
    bounds = [0]
    for n in (per_render if per_render is not None else [rows]):
        bounds.append(bounds[-1] + n)
    R = len(bounds) - 1
    allowed = torch.ones(rows, dtype=torch.bool)
    if special == "unsampled":
        allowed[bounds[1]:bounds[2]] = False                 # render 1: 700 rows, none selected
    cand = allowed.nonzero().squeeze(1)
    sel = cand[torch.randperm(cand.numel(), generator=gen)[:n_sel]].sort().values
    assert sel.numel() == n_sel
    if ctx_mode is None:
        sel_ctx, ctx_rows = None, rows
    elif ctx_mode == "perm":
        ctx_rows = rows + 3
        sel_ctx = torch.randperm(ctx_rows, generator=gen)[:n_sel]
    else:
        ctx_rows = 3 if ctx_mode == "three" else n_sel // 8 + 1
        sel_ctx = torch.randint(0, ctx_rows, (n_sel,), generator=gen)
    ctx = sel if sel_ctx is None else sel_ctx
    x_mean = torch.tensor([0.3, -0.2, 0.05])
    x, mean, scale, Q = [], [], [], []
    for g in range(3):
        small = special == "clamp" and g == 1
        sg = (0.01 + 0.07 * torch.rand(ctx_rows, C[g], generator=gen)) if small else (0.05 + 1.95 * torch.rand(ctx_rows, C[g], generator=gen))
        qg = (1.6e-3 + 0.8e-3 * torch.rand(rows, generator=gen)) if small else (0.05 + 0.95 * torch.rand(rows, generator=gen))
        z = 6 * torch.rand(n_sel, C[g], generator=gen) - 3
        xg = 2 * torch.randn(rows, C[g], generator=gen)
        if small:
            xg = float(x_mean[1]) + 20 * torch.randn(rows, C[g], generator=gen)
            lo, hi, _, _ = rate_sample_bounds(qg.double(), sel, x_mean[g].double(), bounds)
            xs = xg[sel].double()
            for b, sign in ((lo, -1.0), (hi, 1.0)):                       # nothing within 0.1 (3e-3 of the half-width) of a bound
                near = (xs - b.reshape(-1, 1)).abs() < 0.1
                xs = torch.where(near, b.reshape(-1, 1) + sign * 0.2, xs)
            xg[sel] = xs.float()
            xc = torch.minimum(torch.maximum(xg[sel].double(), lo.reshape(-1, 1)), hi.reshape(-1, 1))
            mg = torch.zeros(ctx_rows, C[g])
            mg[ctx] = (xc - z.double() * sg[ctx].double()).float()
        else:
            mg = torch.randn(ctx_rows, C[g], generator=gen)
            off = z * sg[ctx]
            if special == "low":
                pick = torch.rand(n_sel, C[g], generator=gen) < 0.03
                sign = torch.where(torch.rand(n_sel, C[g], generator=gen) < 0.5, -1.0, 1.0)
                far = (6.5 + 1.5 * torch.rand(n_sel, C[g], generator=gen)) * sg[ctx] + 0.5 * qg[sel].reshape(-1, 1)
                off = torch.where(pick, sign * far, off)
            xg[sel] = mg[ctx] + off
        x.append(xg.contiguous()); mean.append(mg.contiguous()); scale.append(sg.contiguous()); Q.append(qg.contiguous())
    mask = (torch.rand(rows, K, generator=gen) > 0.3).float() if with_mask else None
    gS = torch.randn(R, 3, generator=gen)
    gS = torch.where(gS.abs() < 0.1, torch.full_like(gS, 0.5), gS)
    return dict(id=cid, x=x, mean=mean, scale=scale, Q=Q, mask=mask, sel=sel, sel_ctx=sel_ctx, x_mean=x_mean, bounds=bounds, K=K, C=C, R=R,
                rows=rows, ctx_rows=ctx_rows, n_sel=n_sel, gS=gS, special=special)


def rate_sample_facts(c):
    """What the float64 reference says about a case's decisions: per group the unfloored likelihood [n_sel, C], the distance of x
    from the nearer clamp bound in units of the half-width (positive inside), and the per-render counts."""
    d = lambda t: None if t is None else t.double()  # noqa: E731
    _, raws = rate_sample_ref([d(t) for t in c["x"]], [d(t) for t in c["mean"]], [d(t) for t in c["scale"]], [d(t) for t in c["Q"]],
                              d(c["mask"]), c["sel"], c["sel_ctx"], d(c["x_mean"]), c["bounds"], c["K"], with_raw=True)
    margins, counts = [], None
    for g in range(3):
        lo, hi, qm, counts = rate_sample_bounds(c["Q"][g].double(), c["sel"], c["x_mean"][g].double(), c["bounds"])
        xs = c["x"][g][c["sel"]].double()
        half = ((hi - lo) / 2).reshape(-1, 1)
        margins.append(torch.minimum(xs - lo.reshape(-1, 1), hi.reshape(-1, 1) - xs) / half)
    return raws, margins, counts


RN_CASES = [  # (id, rows per render, K, sampling rate, index of a render left without sampled rows or None, all masks zero)
    ("R1-16", [16], 10, 0.5, None, False),
    ("R4-255", [100, 0, 1, 154], 1, 0.3, None, False),
    ("R4-257", [19, 21, 200, 17], 10, 0.3, 2, False),
    ("R16-5000", [310, 290, 0, 333, 305, 1, 299, 320, 311, 317, 300, 303, 330, 325, 309, 947], 10, 0.07, 6, False),
    ("R4-5000-dark", [1200, 1300, 1250, 1250], 10, 0.07, None, True),
    ("R1-257", [257], 1, 0.2, None, False),
]


def rate_normalise_case(case):
    cid, per_render, K, rate, unsampled, dark = case
    gen = torch.Generator().manual_seed(77 + sum(ord(ch) for ch in cid))
    bounds = [0]
    for n in per_render:
        bounds.append(bounds[-1] + n)
    rows, R = bounds[-1], len(per_render)
    om = torch.zeros(rows, K) if dark else (torch.rand(rows, K, generator=gen) < (0.5 if K == 1 else 0.12)).float()
    pick = torch.rand(rows, generator=gen) < rate
    for r in range(R):                       # every render with rows is sampled, the one-row renders included ...
        if per_render[r] > 0:
            pick[bounds[r]] = True
    if unsampled is not None:                # ... but this one
        pick[bounds[unsampled]:bounds[unsampled + 1]] = False
    sel = pick.nonzero().squeeze(1)
    S = torch.rand(R, 3, generator=gen) * 1e4 + 1.0
    g_out, g_sum = torch.randn(R, 4, generator=gen), torch.randn(1, generator=gen)
    return dict(id=cid, bounds=bounds, rows=rows, R=R, K=K, om=om, sel=sel, S=S, g_out=g_out, g_sum=g_sum, dims=(50.0, 6.0, 3.0 * K),
                unsampled=unsampled)


STE_CASES = [  # (id, rows per render, C)
    ("R1-C1", [200], 1),
    ("R3-C3", [65, 0, 64], 3),
    ("R3-C50", [1, 63, 200], 50),
    ("R8-C257", [0, 1, 63, 64, 65, 200, 0, 64], 257),
    ("R8-C3", [200, 65, 64, 63, 1, 0, 64, 0], 3),
]
STE_X_MEAN = 0.37
STE_Q_MODES = {"rows": None, "scalar": 0.125, "scalar02": 0.2}


def ste_case(case, mode):
    """x [rows, C], the steps, x_mean, offs.  mode "rows": a step per row, U(0.05, 0.25) (no powers of two: every product and
    quotient of the statement rounds), but powers of two in {1/16, 1/8, 1/4} on the rows below; "scalar": the one step 1/8;
    "scalar02": the one step 0.2f.  In every render of at least 63 rows: one row clamped above (x / Q = 17 000 ..) and one below; a
    row of ties x = (k + 1/2) Q for k = -4 .. (exact with a power-of-two step, odd and even k: they must round to even); a row of
    positive and negative values whose quotient rounds to 0.  With a step per row the plain rows' steps are nudged (by 0.3 % at a
    time) until x_mean / (the render's mean step) -+ 15000 is further than 2e-2 from an integer."""
    cid, per_render, Cq = case
    per_row = mode == "rows"
    gen = torch.Generator().manual_seed(500 + sum(ord(ch) for ch in cid) + int(per_row))
    offs = [0]
    for n in per_render:
        offs.append(offs[-1] + n)
    rows = offs[-1]
    x = 3 * torch.randn(rows, Cq, generator=gen)
    plain = torch.ones(rows, dtype=torch.bool)
    if per_row:
        Q = 0.05 + 0.2 * torch.rand(rows, generator=gen)
        pow2 = 2.0 ** -torch.randint(2, 5, (rows,), generator=gen).float()
    else:
        Q = torch.full((rows,), STE_Q_MODES[mode])
        pow2 = Q
    k = torch.arange(Cq).float() - 4
    for lo, hi in zip(offs[:-1], offs[1:]):
        if hi - lo >= 63:
            for row in (lo + 5, lo + 17, lo + 23, lo + 31):
                Q[row], plain[row] = pow2[row], False
            x[lo + 5] = (17000.0 + k) * Q[lo + 5]
            x[lo + 17] = (-16000.0 - k) * Q[lo + 17]
            x[lo + 23] = (k + 0.5) * Q[lo + 23]
            x[lo + 31] = torch.where(k.long() % 2 == 0, 0.3, -0.3) * Q[lo + 31] * (1 + k.abs()) / (1 + k.abs()).max()
        if per_row and hi - lo > 1:
            for _ in range(50):
                c = STE_X_MEAN / float(Q[lo:hi].double().mean())
                if min(abs(v - round(v)) for v in (c - 15000.0, c + 15000.0)) > 2e-2:
                    break
                Q[lo:hi] = torch.where(plain[lo:hi], Q[lo:hi] * 1.003, Q[lo:hi])
    return dict(id=cid, x=x.contiguous(), Q=Q.contiguous(), per_row=per_row, x_mean=torch.tensor([STE_X_MEAN]), offs=offs, C=Cq,
                R=len(per_render), rows=rows, exact_ties=mode != "scalar02")


SPECIALS = [0.0, -0.0, 1.0, -1.0, float(np.nextafter(np.float32(1), np.float32(2))), float(np.nextafter(np.float32(1), np.float32(0))),
            float(np.nextafter(np.float32(-1), np.float32(-2))), float(np.nextafter(np.float32(-1), np.float32(0))),
            float(np.float32(1e-45)), float(np.float32(-1e-45)), float("inf"), float("-inf"), float("nan")]


def ste_binary_table(n, seed):
    """n values 0.9 randn with the special values placed around every 4096-entry chunk edge that the table has, at its start and at
    its end (as many as fit)."""
    x = 0.9 * torch.randn(n, generator=torch.Generator().manual_seed(seed))
    sp = torch.tensor(SPECIALS)
    m = sp.numel()
    for start in [0, n - m] + [e - m // 2 for e in range(4096, n + 1, 4096)] + [65536 - m // 2]:
        if 0 <= start and start + m <= n:
            x[start:start + m] = sp
    if 0 < n < m:
        x[:] = sp[:n]
    return x
