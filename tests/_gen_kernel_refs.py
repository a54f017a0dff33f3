"""Plain tensor statements of the 13 entry points of csrc/generate.hip that had no direct test (gsvc_embed_pe, gsvc_gather_rows_forward
/ _backward / _backward_ranked, gsvc_plan_masks, gsvc_plan_scans, gsvc_compact_by_scan, gsvc_ctx_post_forward / _backward,
gsvc_q_rows_forward / _backward, gsvc_segment_rows_sum, gsvc_film_row_maps), written from the header comments of include/gsvc_hip.h
and the kernels' own comments.  Called with float64 they are the references of tests/test_gen_kernels_gpu.py; called with float32
they are "the fp32 tensor statement" those tests calibrate against.  The seeded case builders live here too, so that
tests/test_gen_kernel_refs_cpu.py can pin the statements and assert the cases' preconditions without a GPU.  Nothing here imports
the package under test.

Inputs formed in fp32 BEFORE the arithmetic under test (the contract of each statement):
  embed_pe     xa = fp32(anchor_z) - fp32(cam_z) is ONE fp32 subtraction; the arguments xa * 2^k and cam_z * 2^k are exact in fp32
               (a power-of-two scale).  sin and cos are then taken of those fp32 arguments in the requested dtype.
  gather       every decision sigmoid(m) > 0.01 is taken by the float64 sigmoid of the fp32 input (the cases keep a margin).
  ranked       the feature / offset sums are SEQUENTIAL fp32 sums in view order v = 0 .. 7 started from 0.f, an absent view adding
               0.f (so a lone -0.0 comes out as +0.0); scaling / mask: that sum, THEN one product with the activation factor.
  plan_masks   u <= rate, sum > 0 are fp32 comparisons of fp32 inputs: exact.  The decoded sum adds 0 / 1 values: exact.
  ctx_post     max(scale, fp32(1e-9)), the gates q >= -10, q <= 10, scale >= fp32(1e-9): fp32 comparisons, exact.
  q_rows       raw = 0: out = q_g * adj (one fp32 product); raw = 1: q_g * exp(clamp(v, -10, 10)); the backward's factor is
               q_g * exp(v) inside the gate and exactly 0 outside.
  segment sum  SEQUENTIAL fp32 sum of the run's rows in list order from 0.f, then dst + acc (one fp32 add) when accumulating.
"""
import math

import numpy as np
import torch

from tests._loss_kernel_refs import EPS32, PRINT, err, err_each, ulp_distance  # noqa: F401
from tests._rate_quant_kernel_refs import render_of

LOGIT_001 = math.log(0.01 / 0.99)            # sigmoid(LOGIT_001) = 0.01
MASK_DELTA = 3e-4                            # planted raw masks sit at LOGIT_001 -+ MASK_DELTA: |sigmoid - 0.01| ~ 3e-6
MASK_MARGIN = 1e-6
F32_1EM9 = float(np.float32(1e-9))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def nextafter32(v, towards):
    return float(np.nextafter(np.float32(v), np.float32(towards)))


def sigmoid_margin(m):
    """|sigmoid64(m) - 0.01| per element."""
    return (torch.sigmoid(m.double()) - 0.01).abs()


def clear_of_threshold(m):
    """Raw mask values moved off the sigmoid > 0.01 threshold: anything within 1e-3 of logit(0.01) goes 2e-3 up (a builder's step,
    not a filter: every element of every case is compared)."""
    return torch.where((m - LOGIT_001).abs() < 1e-3, m + 2e-3, m)


# ------------------------------------------------------------------------------------------------------------ embed_pe
EMBED_COUNTS = {
    "four-zero-first-mid": [0, 300, 0, 45],
    "four-zero-mid-last": [150, 0, 77, 0],
    "sixteen-tiny": [0, 1, 2, 3, 3, 2, 1, 0, 0, 0, 3, 1, 2, 0, 1, 3],       # 22 rows: one workgroup spans all 16 for F <= 11
    "sixteen-mixed": [0, 90, 0, 1, 200, 3, 0, 0, 64, 10, 7, 0, 33, 2, 1, 0],
}
EMBED_FREQS = (1, 3, 16, 24)
EMBED_CAMS = [-0.2, 0.0, 0.0125, 0.2, -0.031, 0.11, -0.0625, 0.19, 0.0, -0.17, 0.05, -0.2, 0.2, 0.003, -0.09, 0.14]
EMBED_CASES = [(f"F{F}-{name}", F, name) for F in EMBED_FREQS for name in ("one-partial",) + tuple(EMBED_COUNTS)]


def embed_case(case):
    """anchor [rows, 3] fp32 (only z is read: x and y hold NaN), cam_z fp32 list, bounds [R + 1].  The first row of every render
    sits 0.4 above its camera: |xa| reaches the workload's extent, the largest argument 0.4 * 2^(F - 1)."""
    cid, F, name = case
    counts = [2 * (256 // F) + 1] if name == "one-partial" else EMBED_COUNTS[name]
    R = len(counts)
    bounds = [0]
    for c in counts:
        bounds.append(bounds[-1] + c)
    rows = bounds[-1]
    g = _gen(1000 + F + 7 * R)
    cam = torch.tensor(EMBED_CAMS[:R], dtype=torch.float32) if R > 1 else torch.tensor([-0.2], dtype=torch.float32)
    anchor = torch.full((rows, 3), float("nan"), dtype=torch.float32)
    anchor[:, 2] = (torch.rand(rows, generator=g) - 0.5) * 0.4
    for r in range(R):
        if counts[r]:
            anchor[bounds[r], 2] = cam[r] + 0.4
    return dict(id=cid, F=F, R=R, counts=counts, bounds=bounds, rows=rows, cam=cam, anchor=anchor)


def embed_xa(anchor, cam, bounds):
    """(cam of each row, xa) in fp32: xa is one fp32 subtraction."""
    rows = anchor.shape[0]
    r = render_of(torch.arange(rows, device=anchor.device), bounds)
    cz = cam.to(anchor.device).float()[r]
    return cz, anchor[:, 2].float() - cz


def embed_pe_ref(anchor, cam, bounds, F, dtype):
    """pe [rows, 2 (2 F + 1)] = [cz, sin(cz 2^0), cos(cz 2^0), ..., cos(cz 2^(F-1)) | xa, sin(xa 2^0), ...]."""
    cz, xa = embed_xa(anchor, cam, bounds)
    f = torch.tensor([2.0 ** k for k in range(F)], dtype=torch.float32, device=anchor.device)
    halves = []
    for x in (cz, xa):
        arg = (x.unsqueeze(1) * f).to(dtype)                    # fp32 product by a power of two: exact
        sc = torch.stack([torch.sin(arg), torch.cos(arg)], dim=2).reshape(x.shape[0], 2 * F)
        halves += [x.to(dtype).unsqueeze(1), sc]
    return torch.cat(halves, dim=1)


# ------------------------------------------------------------------------------------------------------------ gather
GATHER_DIMS = [(50, 0, 0), (0, 10, 6), (50, 10, 6), (3, 1, 1)]
GATHER_ROWS = (1, 7, 8, 9, 1000)
GATHER_A = 600


def gather_params(F, K, S, A, seed):
    """The four per-anchor tensors ([A, F], [A, 3 K], [A, S], [A, K]); the raw masks alternate between the two planted values next to
    the threshold in their first two anchors and are random (4 randn, moved off the threshold) elsewhere."""
    g = _gen(seed)
    feat = torch.randn(A, F, generator=g)
    off = torch.randn(A, 3 * K, generator=g)
    scal = torch.randn(A, S, generator=g) * 0.5 - 1.0
    mask = clear_of_threshold(torch.randn(A, K, generator=g) * 4.0)
    if K and A >= 2:
        mask[0] = float(np.float32(LOGIT_001 - MASK_DELTA))
        mask[1] = float(np.float32(LOGIT_001 + MASK_DELTA))
    return feat, off, scal, mask


def gather_case(F, K, S, rows, seed=0):
    """vis [rows]: rows 0 and A - 1 named, repeats; with 1000 rows anchor 5 is hit by 200 of them, the others 0 .. a few times."""
    A = GATHER_A
    g = _gen(31 * rows + F + 3 * K + seed)
    vis = torch.randint(0, A, (rows,), generator=g)
    if rows >= 1000:
        vis[4 + torch.randperm(rows - 4, generator=g)[:200]] = 5
    if rows >= 7:
        vis[0], vis[1], vis[2], vis[3] = 0, A - 1, 1, 1
    else:
        vis[0] = A - 1
    feat, off, scal, mask = gather_params(F, K, S, A, 77 + F + K)
    grads = [torch.randn(rows, w, generator=g) for w in (F, 3 * K, S, K)]
    return dict(F=F, K=K, S=S, A=A, rows=rows, vis=vis, params=[feat, off, scal, mask], grads=grads)


def ste_hard(mask_raw):
    """The hard value of the straight-through mask, decided by the float64 sigmoid of the fp32 input."""
    return (torch.sigmoid(mask_raw.double()) > 0.01)


def gather_fwd_ref(params, vis, decoded, dtype):
    """(feat, offsets, scaling, mask) of the rows: copies; scaling exp(raw); mask the hard 0 / 1 value (the kernel forms
    (h - s) + s, which the test holds within 1 ulp of h)."""
    feat, off, scal, mask = (p.to(dtype)[vis] for p in params)
    if not decoded:
        scal = torch.exp(scal)
        mask = ste_hard(params[3])[vis].to(dtype)
    return feat, off, scal, mask


def gather_factors(params, decoded, dtype):
    """Per-anchor activation derivatives of the scaling and mask groups: exp(raw), s (1 - s); 1 when decoded."""
    scal, mask = params[2].to(dtype), params[3].to(dtype)
    if decoded:
        return torch.ones_like(scal), torch.ones_like(mask)
    s = torch.sigmoid(mask)
    return torch.exp(scal), s * (1 - s)


def gather_bwd_ref(params, vis, grads, decoded, dtype):
    """Dense gradients [A, W] of the four groups and the scale of each element (the sum of the |terms| that meet in it):
    d[v] += g[row] * factor[v] per row (the atomic kernel's order of operations)."""
    A = params[0].shape[0]
    fs, fm = gather_factors(params, decoded, dtype)
    out, scale = [], []
    for k, g in enumerate(grads):
        t = g.to(dtype)
        if k == 2:
            t = t * fs[vis]
        if k == 3:
            t = t * fm[vis]
        z = torch.zeros(A, g.shape[1], dtype=dtype, device=g.device)
        out.append(z.index_add(0, vis, t))
        scale.append(z.index_add(0, vis, t.abs()))
    return out, scale


# ------------------------------------------------------------------------------------------------------------ ranked backward
RANKED_R = (0, 1, 2, 8)
RANKED_A = (1, 63, 64, 65, 1000)
RANKED_PATTERNS = {0: ("none",), 1: ("random",), 2: ("empty-full",), 8: ("none-all", "empty-full")}
RANKED_DIMS = (50, 10, 6)
# the group subsets of the entry's two callers (features alone, with NULL scaling_p / mask_p; offsets, scaling and masks), at a few
# (R, A, pattern): the kernel's column dispatch item / CT runs with F = 0 and with K = S = 0
RANKED_SUBSET_DIMS = [(50, 0, 0), (0, 10, 6)]
RANKED_SUBSET_SHAPES = [(0, 64, "none"), (1, 63, "random"), (2, 65, "empty-full"), (8, 1000, "none-all")]


def ranked_seen(R, A, pattern, seed):
    """seen [R, A] bool.  "empty-full": view R // 4 empty, view R - 1 - R // 4 full ... ; "none-all": anchor 0 in no view, anchor
    A - 1 in all (A = 1: in all)."""
    g = _gen(seed)
    seen = torch.rand(R, A, generator=g) < 0.4
    if pattern == "empty-full":
        seen[R // 4] = False
        seen[R - 1 - R // 4] = True
    if pattern == "none-all":
        seen[:, 0] = False
        seen[:, A - 1] = True
    return seen


def ranked_case(R, A, pattern, dims=RANKED_DIMS):
    """seen, rank, vis of R views over A anchors, the four per-anchor tensors and the rows' gradients; a group whose width in
    ``dims`` = (F, K, S) is 0 has empty tensors (the entry then gets NULL pointers for it)."""
    F, K, S = dims
    seed = 1 + 13 * R + A
    seen = ranked_seen(R, A, pattern, seed)
    rank = torch.cumsum(seen.reshape(-1).long(), 0)
    rows = int(seen.sum())
    vis = torch.cat([s.nonzero().squeeze(1) for s in seen]) if R else torch.zeros(0, dtype=torch.long)
    g = _gen(seed + 5)
    params = gather_params(F, K, S, A, seed + 9)
    grads = [torch.randn(rows, w, generator=g) for w in (F, 3 * K, S, K)]
    for t in grads[:2]:
        if t.numel():
            t[:, 0] = -0.0                  # a column of -0.0: 0.f + (-0.0) = +0.0, whatever the number of views
    return dict(R=R, A=A, F=F, K=K, S=S, rows=rows, seen=seen, rank=rank, vis=vis, params=list(params), grads=grads, pattern=pattern)


def ranked_view_terms(seen, rank, g, dtype):
    """[8, A, W]: the gradient row of anchor a in view v, 0 where the view does not hold it (views past R: zeros)."""
    R, A = seen.shape
    W = g.shape[1]
    out = torch.zeros(8, A, W, dtype=dtype, device=g.device)
    for v in range(R):
        a = seen[v].nonzero().squeeze(1)
        out[v, a] = g.to(dtype)[rank.view(R, A)[v, a] - 1]
    return out


def ranked_sum(seen, rank, g, dtype):
    """Sequential sum over the 8 slots in view order from 0 (in fp32 this is the kernel's order, bit for bit)."""
    terms = ranked_view_terms(seen, rank, g, dtype)
    acc = torch.zeros_like(terms[0])
    for v in range(8):
        acc = acc + terms[v]
    return acc, terms.abs().sum(0)


def ranked_bwd_ref(c, decoded, dtype, dev=None):
    """(dense gradients of the four groups, their scales): sum in view order, then the activation factor."""
    mv = (lambda t: t.to(dev)) if dev is not None else (lambda t: t)
    seen, rank = mv(c["seen"]), mv(c["rank"])
    params = [mv(p) for p in c["params"]]
    fs, fm = gather_factors(params, decoded, dtype)
    out, scale = [], []
    for k, g in enumerate(c["grads"]):
        acc, mag = ranked_sum(seen, rank, mv(g), dtype)
        if k == 2:
            acc, mag = acc * fs, mag * fs.abs()
        if k == 3:
            acc, mag = acc * fm, mag * fm.abs()
        out.append(acc)
        scale.append(mag)
    return out, scale


# ------------------------------------------------------------------------------------------------------------ plan masks
PLAN_R = (1, 4, 16)
PLAN_A = (1, 255, 256, 257, 3000)
PLAN_K = (1, 10)
PLAN_RATE = float(np.float32(0.05))


def plan_masks_case(R, A, K, decoded, rate0=False):
    """Views [R, A] (bytes 0 / 1), mask_raw [A, K], u [R, A], rate.  Planted: u.flat[0] = rate (its anchor visible and live:
    chosen), u.flat[1] = nextafter(rate, +inf) (visible and live: NOT chosen).  rate0: rate = 0 and every third u exactly 0.
    Raw masks take only the two values logit(0.01) -+ MASK_DELTA, one on either side of the threshold.  For K >= 2 every row holds
    both (column 0 below, column 1 above, the other columns above with probability 0.3) EXCEPT the 40 % of the rows that are below
    throughout: "each row given both values" alone would make every anchor live and leave the `not live` branch of the raw mode
    without a case, so the builder adds those rows.  A row of K = 1 holds a single value, below (40 %) or above.  A planted anchor's
    column 0 is set above as well (it has to be live whatever its row was).  Decoded masks are 0 / 1: a third of the rows all zero,
    a third one-hot, the rest random."""
    g = _gen(17 * R + A + 3 * K + decoded + (1000 if rate0 else 0))
    vis = (torch.rand(R, A, generator=g) < 0.5).to(torch.uint8)
    if decoded:
        kind = torch.randint(0, 3, (A,), generator=g)
        onehot = torch.zeros(A, K)
        onehot[torch.arange(A), torch.randint(0, K, (A,), generator=g)] = 1.0
        rnd = (torch.rand(A, K, generator=g) < 0.5).float()
        mask = torch.where((kind == 0).unsqueeze(1), torch.zeros(A, K), torch.where((kind == 1).unsqueeze(1), onehot, rnd))
    else:
        dead = (torch.rand(A, 1, generator=g) < 0.4).expand(A, K)
        up = torch.rand(A, K, generator=g) < 0.3
        if K >= 2:
            up[:, 0], up[:, 1] = False, True
        else:
            up[:] = True
        up &= ~dead
        lo, hi = np.float32(LOGIT_001 - MASK_DELTA), np.float32(LOGIT_001 + MASK_DELTA)
        mask = torch.where(up, torch.full((A, K), float(hi)), torch.full((A, K), float(lo)))
    rate = 0.0 if rate0 else PLAN_RATE
    u = torch.rand(R, A, generator=g)
    u = torch.where(u == rate, u + 0.5, u)                 # the only u == rate are the planted ones
    planted = []
    if rate0:
        u.view(-1)[::3] = 0.0
    else:
        flat = u.view(-1)
        flat[0] = rate
        planted.append(0)
        if R * A >= 2:
            flat[1] = nextafter32(rate, np.inf)
            planted.append(1)
        for j in planted:
            r, a = divmod(j, A)
            vis[r, a] = 1
            if decoded:
                mask[a] = 0.0
                mask[a, K - 1] = 1.0
            else:
                mask[a, 0] = float(np.float32(LOGIT_001 + MASK_DELTA))
    return dict(R=R, A=A, K=K, decoded=decoded, vis=vis, mask=mask.float(), u=u.float(), rate=rate, planted=planted)


def plan_live(mask, decoded):
    if decoded:
        s = torch.zeros(mask.shape[0], dtype=torch.float32, device=mask.device)
        for k in range(mask.shape[1]):
            s = s + mask[:, k]
        return s > 0
    return (torch.sigmoid(mask.double()) > 0.01).any(dim=1)


def plan_masks_ref(vis, mask, u, rate, decoded, with_chosen=True):
    """(M [R, A], present [A], chosen [R, A] or None) as uint8."""
    M = (vis != 0)
    present = M.any(dim=0)
    chosen = None
    if with_chosen:
        rate32 = torch.tensor(rate, dtype=torch.float32, device=u.device)
        chosen = (M & plan_live(mask, decoded).unsqueeze(0) & (u <= rate32)).to(torch.uint8)
    return M.to(torch.uint8), present.to(torch.uint8), chosen


# ------------------------------------------------------------------------------------------------------------ plan scans
SCAN_SHAPES = [("A1-R1", 1, 1, "random"), ("A1-R3", 3, 1, "full"), ("below-16", 3, 5, "random"), ("two-chunks-full", 2, 4096, "full"),
               ("one-chunk-full", 1, 4096, "full"), ("chunk-edge", 3, 1367, "random"), ("general", 4, 3000, "random"),
               ("empty", 2, 300, "empty")]
SCAN_OFFSETS = [(0, 0, 0), (1, 8, 15), (8, 15, 1), (15, 1, 8)]


def plan_scans_case(case):
    """View masks [R, A] (bytes 0 / 1: the header's contract), chosen a subset of them, present their union."""
    cid, R, A, fill = case
    g = _gen(R * 7 + A)
    if fill == "full":
        M = torch.ones(R, A, dtype=torch.bool)
    elif fill == "empty":
        M = torch.zeros(R, A, dtype=torch.bool)
    else:
        M = torch.rand(R, A, generator=g) < 0.45
        if A == 1:
            M[:] = True
    chosen = M & (torch.rand(R, A, generator=g) < (1.0 if fill == "full" else 0.3))
    return dict(id=cid, R=R, A=A, M=M.to(torch.uint8), chosen=chosen.to(torch.uint8), present=M.any(dim=0).to(torch.uint8))


def plan_scans_ref(M, chosen, present):
    """scan [R A], flat, sel_rows (None without chosen), pos [A], distinct, counts [R + 2]; lists at their true length."""
    R, A = M.shape
    m = M.reshape(-1) != 0
    scan = torch.cumsum(m.long(), 0)
    flat = m.nonzero().squeeze(1) % A
    sel = None if chosen is None else scan[chosen.reshape(-1) != 0] - 1
    p = present != 0
    pos = torch.cumsum(p.long(), 0) - 1
    distinct = p.nonzero().squeeze(1)
    counts = torch.cat([scan.view(R, A)[:, -1], torch.tensor([0 if sel is None else sel.numel(), distinct.numel()], device=M.device)])
    return scan, flat, sel, pos, distinct, counts


def compact_ref(mask, value, bias):
    idx = (mask != 0).nonzero().squeeze(1)
    return idx if value is None else value[idx] + bias


# ------------------------------------------------------------------------------------------------------------ context tail
CTX_Q_PLANTS = [10.0, -10.0, nextafter32(10.0, np.inf), nextafter32(-10.0, -np.inf), 50.0, -50.0]
CTX_S_PLANTS = [F32_1EM9, nextafter32(F32_1EM9, 0.0), 0.0, -0.5, -F32_1EM9]
CTX_SHAPES = [(n, C) for C in (1, 30) for n in (1, 9, 4097)]


def ctx_post_case(n, C):
    """params [n, 2 C], q [n] and three upstream gradients.  q starts with as many of CTX_Q_PLANTS as fit (n = 1: +10 for C = 1,
    -10 for C = 30), the flattened scale half of params with as many of CTX_S_PLANTS as fit; the rest of q is 8 randn (a fifth
    beyond +-10), every seventh scale row is -0.5."""
    g = _gen(100 * C + n)
    params = torch.randn(n, 2 * C, generator=g)
    q = torch.randn(n, generator=g) * 8
    params[::7, C:] = -0.5
    plants = CTX_Q_PLANTS if (n > 1 or C == 1) else CTX_Q_PLANTS[1:]
    nq = min(n, len(plants))
    q[:nq] = torch.tensor(plants[:nq], dtype=torch.float32)
    ns = min(n * C, len(CTX_S_PLANTS))
    sc = params[:, C:].clone().reshape(-1)
    sc[:ns] = torch.tensor(CTX_S_PLANTS[:ns], dtype=torch.float32)
    params[:, C:] = sc.view(n, C)
    gm, gs, ga = torch.randn(n, C, generator=g), torch.randn(n, C, generator=g), torch.randn(n, generator=g)
    return dict(n=n, C=C, params=params, q=q, g_mean=gm, g_scale=gs, g_adj=ga, nq=nq, ns=ns, q_plants=plants[:nq])


def ctx_post_fwd_ref(params, q, dtype):
    C = params.shape[1] // 2
    floor = torch.tensor(F32_1EM9, dtype=torch.float32, device=params.device)
    mean, scale = params[:, :C].to(dtype), torch.maximum(params[:, C:], floor).to(dtype)       # fp32 max: exact
    return mean, scale, torch.exp(torch.clamp(q, -10.0, 10.0).to(dtype))


def ctx_post_gates(params, q):
    """(scale gate [n, C], q gate [n]) as bool: gradient passes at exactly 1e-9f and at exactly +-10."""
    C = params.shape[1] // 2
    floor = torch.tensor(F32_1EM9, dtype=torch.float32, device=params.device)
    return params[:, C:] >= floor, (q >= -10.0) & (q <= 10.0)


def ctx_post_bwd_ref(params, q, adj, g_mean, g_scale, g_adj):
    """(dparams [n, 2 C], dq [n]) in fp32 given the forward's adj; a None gradient gives exact zeros.  Every value is a copy, a
    zero or ONE fp32 product: exact."""
    n, C = params.shape[0], params.shape[1] // 2
    sg, qg = ctx_post_gates(params, q)
    z = torch.zeros(n, C, dtype=torch.float32, device=params.device)
    dm = z if g_mean is None else g_mean
    ds = z if g_scale is None else torch.where(sg, g_scale, z)
    dq = z[:, 0] if g_adj is None else torch.where(qg, g_adj * adj, z[:, 0])
    return torch.cat([dm, ds], dim=1), dq


# ------------------------------------------------------------------------------------------------------------ q rows
Q_BASE = tuple(float(np.float32(v)) for v in (0.3, 0.011, 1.7))
Q_PLANTS = [10.0, -10.0, nextafter32(10.0, np.inf), nextafter32(-10.0, -np.inf), 30.0, -30.0]
Q_ROWS = (1, 255, 257, 2500)


def q_rows_case(rows, D, mapped, raw):
    """adj [3, D] (raw: 4 randn with the six planted values in slots 0 .. 5 of each group when D >= 6, else 3 randn; not raw:
    positive steps), ctx_row [rows] (slot D - 1 named by no row when D > 6, slots 0 .. 5 each by some row) or None (D = rows),
    g [3, rows]."""
    if not mapped:
        D = rows
    g = _gen(rows * 3 + D + 2 * raw + mapped)
    if raw:
        adj = torch.randn(3, D, generator=g) * (4.0 if D >= 6 else 3.0)
        if D >= 6:
            for k in range(3):
                adj[k, :6] = torch.tensor(Q_PLANTS[k:] + Q_PLANTS[:k], dtype=torch.float32)
    else:
        adj = torch.rand(3, D, generator=g) + 0.5
    ctx = None
    if mapped:
        ctx = torch.randint(0, max(D - 1, 1), (rows,), generator=g)
        if D > 6 and rows >= 12:
            ctx[:12] = torch.arange(12) % 6
    grads = torch.randn(3, rows, generator=g)
    return dict(rows=rows, D=D, raw=raw, adj=adj.float(), ctx=ctx, g=grads)


def q_adj_ref(v, dtype):
    return torch.exp(torch.clamp(v, -10.0, 10.0).to(dtype))


def q_rows_fwd_ref(adj, ctx, raw, dtype):
    """out [3, rows]."""
    a = adj if ctx is None else adj[:, ctx]
    val = q_adj_ref(a, dtype) if raw else a.to(dtype)
    qb = torch.tensor(Q_BASE, dtype=torch.float32, device=adj.device).to(dtype).view(3, 1)
    return qb * val


def q_rows_bwd_ref(adj, ctx, raw, g, present, dtype):
    """(grad_adj [3, D], scale [3, D]): per row the term (q_g * factor) * g, factor = exp(v) [|v| <= 10] when raw else 1; with a map
    the rows of a slot are added; a group whose gradient is absent gives zeros."""
    D = adj.shape[1]
    a = adj if ctx is None else adj[:, ctx]
    qb = torch.tensor(Q_BASE, dtype=torch.float32, device=adj.device).to(dtype).view(3, 1)
    f = qb.expand_as(a)
    if raw:
        gate = (a >= -10.0) & (a <= 10.0)
        f = torch.where(gate, qb * torch.exp(a.to(dtype)), torch.zeros((), dtype=dtype, device=adj.device))
    t = f * g.to(dtype)
    t = t * torch.tensor([1.0 if p else 0.0 for p in present], dtype=dtype, device=adj.device).view(3, 1)
    if ctx is None:
        return t, t.abs()
    z = torch.zeros(3, D, dtype=dtype, device=adj.device)
    return z.index_add(1, ctx, t), z.index_add(1, ctx, t.abs())


# ------------------------------------------------------------------------------------------------------------ segment rows sum
SEG_C = (1, 3, 50)
SEG_N = (1, 86, 1000)
SEG_TARGETS = ("distinct", "equal", "mixed")


def segment_case(n, C, kind):
    """src [n, C], targets idx [n] among T rows (T > every target + 1: the last row and, for "mixed", the odd rows are named by
    no run), their stable sort (sorted_idx, order) and a known non-zero dst [T, C]."""
    g = _gen(n * 5 + C + len(kind))
    T = 2 * n + 3
    if kind == "distinct":
        idx = torch.randperm(n, generator=g)
    elif kind == "equal":
        idx = torch.full((n,), 2, dtype=torch.long)
    else:
        idx = 2 * torch.randint(0, max(n // 8, 1), (n,), generator=g)
    sorted_idx, order = torch.sort(idx, stable=True)
    return dict(n=n, C=C, T=T, idx=idx, sorted_idx=sorted_idx, order=order, src=torch.randn(n, C, generator=g),
                dst=torch.rand(T, C, generator=g) + 1.0)


def segment_rows_sum_f32(c, accumulate, dst):
    """dst after the call, in fp32 bit for bit: per target the rows of its run added one by one in list order from 0.f, then
    written, or added to dst with one fp32 add; other rows of dst as they were.  (numpy float32: every add rounds once.)"""
    src, order, t = c["src"].numpy(), c["order"].numpy(), c["sorted_idx"].numpy()
    acc = np.zeros((c["T"], c["C"]), dtype=np.float32)
    for p in range(c["n"]):
        acc[t[p]] = acc[t[p]] + src[order[p]]
    out = dst.copy()
    named = np.unique(t)
    out[named] = (dst[named] + acc[named]) if accumulate else acc[named]
    return out, named


# ------------------------------------------------------------------------------------------------------------ film row maps
FILM_CASES = [("R2-A1", 2, 1, "full"), ("R2-empty-vs-full", 2, 40, "empty-full"), ("R2-random", 2, 500, "random"),
              ("R2-both-empty", 2, 30, "empty"), ("R16-sparse", 16, 300, "sparse"), ("R16-random", 16, 257, "random"), ("R16-A1", 16, 1, "random")]


def film_case(case):
    """View masks [R, A] and everything gsvc_plan_scans derives from them.  "sparse": only views 2, 3 and 9 hold anchors (three pairs
    are empty on both sides, view 8 is empty opposite view 9), so rows < (R / 2) D."""
    cid, R, A, fill = case
    g = _gen(R + 3 * A)
    M = torch.rand(R, A, generator=g) < 0.4
    if fill == "full":
        M[:] = True
    if fill == "empty":
        M[:] = False
    if fill == "empty-full":
        M[0], M[1] = False, True
    if fill == "sparse":
        keep = torch.zeros(R, dtype=torch.bool)
        keep[[2, 3, 9]] = True
        M &= keep.unsqueeze(1)
        M[9] = True
    if fill == "random" and R == 16:
        M[4], M[5] = False, False                     # a pair of views that are both empty
        M[6], M[7] = False, True                      # an empty view opposite a full one
    scan, flat, _, pos, distinct, counts = plan_scans_ref(M.to(torch.uint8), None, M.any(dim=0).to(torch.uint8))
    bounds = [0] + [int(v) for v in counts[:R]]
    return dict(id=cid, R=R, A=A, M=M.to(torch.uint8), vis=flat, bounds=bounds, rows=bounds[-1], pos=pos, distinct=distinct,
                D=int(distinct.numel()), scan=scan)


def film_row_maps_ref(c):
    """(row_of [rows], src_a, src_b [(R / 2) D]) as int32, by the index statement of the header."""
    R, A, D = c["R"], c["A"], c["D"]
    rows = c["rows"]
    view = render_of(torch.arange(rows), c["bounds"])
    row_of = c["pos"][c["vis"]] + (view // 2) * D
    M, scan = c["M"].view(R, A), c["scan"].view(R, A)
    d = c["distinct"]
    src = []
    for side in (0, 1):
        v = torch.arange(R // 2) * 2 + side
        s = torch.where(M[v][:, d] != 0, scan[v][:, d] - 1, torch.full((R // 2, D), -1, dtype=torch.long))
        src.append(s.reshape(-1).to(torch.int32))
    return row_of.to(torch.int32), src[0], src[1]
