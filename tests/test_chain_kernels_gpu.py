"""The whole-network chain kernels (csrc/mlp_chain.hip) through their C entry points — gsvc_generate_all_forward / _backward and
gsvc_quant_step_nets_forward / _backward, called through ctypes on raw buffers — each against the float64 run of its plain tensor
statement in tests/_chain_kernel_refs.py.  No module of the package stands between the test and the kernels, so nothing here can fall
back to torch.

Every tensor that crosses HBM is looked at by name: cg, cb, gamma, beta, a1, h, x3, y; go, gh, gz1, gbeta, ggamma, gcg, gcb, the
generators' feature-gradient parts and their fourteen weight / bias gradients; z1 .. a4, y, g4 .. g1, gfeat_sum and the ten gradients
of the deformation network; z, a, q, dz, dX of the quant_step networks.

One entry, one check: the backward's reference is evaluated on what the backward kernel is handed — the forward's own `saved` and y,
cast up to float64 (test-made integers in the exact probe) — so a forward error cannot leak into the backward's verdict, and the FiLM
ReLU mask [cg > 0] is the mask of the tensor the kernel reads.  No element is left out of any comparison.

Assertions per case:
  * exact probe ("lin"): the linear-regime integer probe of _chain_kernel_refs (every GELU pre-activation >= 8, where the kernels'
    GELU is the identity and its derivative 1 in fp32; sums of absolute terms below 2^24: tests/test_chain_kernel_refs_cpu.py shows
    both for every case used here): every stored tensor equals the integer float32(round(ref64)) (as values: a zero's sign is not compared, except for
    the summed d gamma / d beta of a FiLM row with neither side, which must be +0);
  * single non-zero ("one", "one_cond"): one path of weights to the last row's last output, through each chain's last product and
    once through the condition half of the deformation network's first layer;
  * float64 rule ("randn"): e_kernel <= 4 e32 + 4 L eps32 for every tensor, e = max |got - ref64| / S element by element, S the
    carried sum of absolute terms, L the number of products behind the tensor, e32 the error of the same statement run in fp32 on
    the GPU.  GSVC_PRINT_ERRORS=1 prints both errors per tensor and case.  The carried scale grows with the depth of the chain, so
    every stored tensor is also held, by the same rule with L = 1, against the statement of its own step evaluated on the stored
    tensors that step read (the "step" lines).

Every output, saved and scratch buffer is pre-filled with a NaN pattern no finite input produces, with guard floats behind: every
named region must be fully written, everything else in the buffer (but the weight gradients' workspace) and the guards must survive.
"""
import ctypes as C

import pytest
import torch

from tests import _chain_kernel_refs as R
from tests._chain_kernel_refs import COND, DEF_OUT, EPS32, FEAT, HID, PRINT, err

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF            # a quiet NaN with a payload
PAD = 64
OK, E_INVALID, E_UNSUPPORTED = 0, -1, -3
f64, f32 = torch.float64, torch.float32
GEN_GRADS = R.GEN_W              # the fields of gsvc_generator_grads; the statements call them "d" + name


def _lib():
    from gsvc_amd import _lib
    return _lib, _lib.lib(), _lib.current_stream()


class Buf:
    """n floats of sentinels in an aligned allocation, PAD more behind."""

    def __init__(self, n):
        self.n = int(n)
        self.bits = torch.full((self.n + PAD,), SENTINEL, dtype=torch.int32, device="cuda")
        self.ptr = self.bits.data_ptr()
        assert self.ptr % 16 == 0

    @property
    def f(self):
        return self.bits.view(f32)[:self.n]

    def untouched(self):
        return bool((self.bits == SENTINEL).all())

    def only_written(self, regions, free=()):
        """Every (offset, count) region holds no sentinel; everything else but the `free` regions (where anything goes) holds nothing
        else, the PAD floats behind included."""
        rest = torch.ones(self.n + PAD, dtype=torch.bool, device="cuda")
        for off, cnt in regions:
            if not bool((self.bits[off:off + cnt] != SENTINEL).all()):
                return False
            rest[off:off + cnt] = False
        for off, cnt in free:
            rest[off:off + cnt] = False
        return bool((self.bits[rest] == SENTINEL).all())

    def written(self):
        return self.only_written([(0, self.n)])

    def views(self, layout, base=0):
        return {k: self.f[base + o:base + o + r * c].view(r, c) for k, (o, r, c) in layout.items()}


def _regions(layout, base=0):
    return [(base + o, r * c) for o, r, c in layout.values()]


def _ptrs(ps):
    return (C.c_void_p * len(ps))(*ps)


# ------------------------------------------------------------------------------------------------------------ comparisons
def _compare(tag, got, r64, r32):
    """got {name: tensor} against the float64 statement {name: (value, scale, L)}: equal to R.exact_value(value) when r32 is None (the
    exact probes), else the float64 rule with e32 from the fp32 statement r32."""
    for name, (v, S, L) in r64.items():
        g = got[name]
        assert g.shape == v.shape, (tag, name, g.shape, v.shape)
        if r32 is None:
            assert torch.equal(g, R.exact_value(v)), (tag, name, int((g != R.exact_value(v)).sum()), "elements differ from the float64 result")
            continue
        e_k, e32 = err(g, v, S), err(r32[name][0], v, S)
        if PRINT:
            print(f"CHAIN_ERR {tag} {name}: kernel {e_k:.3e} fp32 statement {e32:.3e} L {L}")
        assert e_k <= 4 * e32 + 4 * L * EPS32, (tag, name, e_k, e32, L)


def _single(tag, y, value):
    """y is zero but for y[last row][last column] = value."""
    want = torch.zeros_like(y)
    want[-1, -1] = value
    assert torch.equal(y, want), (tag, y.nonzero().tolist()[:8])


# ------------------------------------------------------------------------------------------------------------ one call pair
class Pass:
    """The arguments and sentinel buffers of one gsvc_generate_all_forward / _backward pair for a case of R.build_case."""

    def __init__(self, c, bwd_acts=None):
        self.lb, self.L, self.st = _lib()
        lb, L = self.lb, self.L
        self.c = c
        self.d = d = R.cast(c, f32, "cuda")
        self.M, self.n = c["feat"].shape[0], len(c["nets"])
        self.film = d["film"]
        self.Mf = self.film["cond"].shape[0] if self.film else self.M
        M, n, Mf = self.M, self.n, self.Mf
        self.outs = [net["out"] for net in c["nets"]]
        self.nets = self._gen_structs([net["act"] for net in c["nets"]])
        self.nets_bwd = self._gen_structs(bwd_acts) if bwd_acts else self.nets
        self.deform = lb.DeformNetC()
        for i in range(5):
            self.deform.W[i], self.deform.b[i] = d["deform"]["W"][i].data_ptr(), d["deform"]["b"][i].data_ptr()
        self.deform.feat_dim, self.deform.cond_dim, self.deform.hidden_dim, self.deform.out_dim = FEAT, COND, HID, DEF_OUT
        self.film_c = None
        if self.film:
            f = self.film
            self.film_c = lb.FilmRowsC(Mf, f["cond"].data_ptr(), f["row_of"].data_ptr(), f["src_a"].data_ptr(), f["src_b"].data_ptr())
        fr = Mf if self.film else 0
        # sizes: the library's, checked against the header's formulas and the layout helper
        self.saved_floats = [L.gsvc_generator_saved_floats(C.byref(self.nets[i]), M, fr) for i in range(n)] + [L.gsvc_deform_saved_floats(C.byref(self.deform), M)]
        self.inf_floats = [L.gsvc_generator_inference_floats(C.byref(self.nets[i]), M, fr) for i in range(n)] + [L.gsvc_deform_inference_floats(C.byref(self.deform), M)]
        self.scratch_floats = [L.gsvc_generator_scratch_floats(C.byref(self.nets[i]), M, fr) for i in range(n)]
        self.scratch_deform_floats = L.gsvc_deform_scratch_floats(C.byref(self.deform), M)
        for i in range(n):
            assert self.saved_floats[i] == R.gen_saved_floats(M, Mf) and self.inf_floats[i] == R.gen_inference_floats(M, Mf)
            assert R.gen_saved_layout(M, Mf)[1] <= self.saved_floats[i] and R.gen_saved_layout(M, Mf, True)[1] <= self.inf_floats[i]
            assert R.gen_scratch_layout(M, Mf, self.outs[i])[1] <= R.gen_scratch_floats_min(M, Mf, self.outs[i]) <= self.scratch_floats[i]
        assert self.saved_floats[n] == R.deform_saved_floats(M) == R.deform_saved_layout(M)[1] and self.inf_floats[n] == R.deform_inference_floats(M)
        assert R.deform_scratch_layout(M)[1] <= R.deform_scratch_floats_min(M) <= self.scratch_deform_floats
        self.new_forward_buffers()
        self.new_backward_buffers()

    def _gen_structs(self, acts):
        arr = (self.lb.GeneratorNetC * 3)()
        for i, net in enumerate(self.d["nets"]):
            for k in R.GEN_W:
                setattr(arr[i], k, net[k].data_ptr())
            arr[i].feat_dim, arr[i].cond_dim, arr[i].hidden_dim, arr[i].out_dim, arr[i].out_act = FEAT, COND, HID, net["out"], acts[i]
        return arr

    # ---- forward
    def new_forward_buffers(self):
        self.saved = [Buf(s) for s in self.saved_floats]
        self.y = [Buf(self.M * o) for o in self.outs + [DEF_OUT]]

    def forward(self, keep=1, **over):
        a = dict(nets=self.nets, n=self.n, deform=C.byref(self.deform), feat=self.d["feat"].data_ptr(), cond=self.d["cond"].data_ptr(), M=self.M,
                 film=C.byref(self.film_c) if self.film_c else None, saved=_ptrs([b.ptr for b in self.saved]), y=_ptrs([b.ptr for b in self.y]))
        a.update(over)
        rc = self.L.gsvc_generate_all_forward(a["nets"], a["n"], a["deform"], a["feat"], a["cond"], a["M"], a["film"], a["saved"], a["y"], keep, self.st)
        torch.cuda.synchronize()
        return rc

    def saved_layout(self, i, inference=False):
        return R.deform_saved_layout(self.M, inference)[0] if i == self.n else R.gen_saved_layout(self.M, self.Mf, inference)[0]

    def forward_got(self, inference=False):
        """Checks that the forward wrote its regions and nothing else; [{name: tensor}] per network, the deformation network last."""
        got = []
        for i in range(self.n + 1):
            lay = self.saved_layout(i, inference)
            assert self.saved[i].only_written(_regions(lay)), ("saved", i, inference)
            assert self.y[i].written(), ("y", i)
            g = self.saved[i].views(lay)
            g["y"] = self.y[i].f.view(self.M, -1)
            got.append(g)
        return got

    # ---- backward
    def new_backward_buffers(self):
        M, n = self.M, self.n
        self.scratch_base = [0]
        for s in self.scratch_floats:
            self.scratch_base.append(self.scratch_base[-1] + (s + 3) // 4 * 4)
        self.scratch = Buf(self.scratch_base[-1])
        self.scratch_deform = Buf(self.scratch_deform_floats)
        self.gfeat_sum = Buf(M * FEAT)
        self.parts = [Buf(M * FEAT) for _ in range(n)]
        self.gen_grads = [{k: Buf(self.d["nets"][i][k].numel()) for k in GEN_GRADS} for i in range(n)]
        self.def_grads = {"W": [Buf(w.numel()) for w in self.d["deform"]["W"]], "b": [Buf(b.numel()) for b in self.d["deform"]["b"]]}
        self.gg_c = (self.lb.GeneratorGradsC * 3)()
        for i in range(n):
            for k in GEN_GRADS:
                setattr(self.gg_c[i], k, self.gen_grads[i][k].ptr)
        self.dg_c = self.lb.DeformGradsC()
        for i in range(5):
            self.dg_c.W[i], self.dg_c.b[i] = self.def_grads["W"][i].ptr, self.def_grads["b"][i].ptr

    def backward_buffers(self):
        return ([self.scratch, self.scratch_deform, self.gfeat_sum] + self.parts + [b for g in self.gen_grads for b in g.values()] +
                self.def_grads["W"] + self.def_grads["b"])

    def backward(self, y, gy, wgrad_stream=None, **over):
        """y: n tensors (the generators' outputs), gy: n + 1 tensors."""
        self.alive = (y, gy)      # the kernels read them until the synchronize below
        a = dict(nets=self.nets_bwd, n=self.n, deform=C.byref(self.deform), feat=self.d["feat"].data_ptr(), cond=self.d["cond"].data_ptr(), M=self.M,
                 film=C.byref(self.film_c) if self.film_c else None, saved=_ptrs([b.ptr for b in self.saved]),
                 y=_ptrs([t.data_ptr() for t in y]), gy=_ptrs([t.data_ptr() for t in gy]), scratch=self.scratch.ptr,
                 scratch_deform=self.scratch_deform.ptr, gfeat_sum=self.gfeat_sum.ptr, parts=_ptrs([b.ptr for b in self.parts]))
        a.update(over)
        rc = self.L.gsvc_generate_all_backward(a["nets"], a["n"], a["deform"], a["feat"], a["cond"], a["M"], a["film"], a["saved"], a["y"], a["gy"],
                                               a["scratch"], a["scratch_deform"], a["gfeat_sum"], a["parts"], self.gg_c, C.byref(self.dg_c), self.st,
                                               wgrad_stream)
        torch.cuda.synchronize()
        return rc

    def backward_got(self):
        """Checks that the backward wrote its regions and nothing else; ([{name: tensor}] per generator, {name: tensor} of the
        deformation network)."""
        M, n, Mf = self.M, self.n, self.Mf
        regions, free, gens = [], [], []
        for i in range(n):
            lay, end = R.gen_scratch_layout(M, Mf, self.outs[i])
            base = self.scratch_base[i]
            regions += _regions(lay, base)
            # the rest of the network's region is the weight gradients' workspace: anything goes there
            free.append((base + end, self.scratch_base[i + 1] - base - end))
            g = self.scratch.views(lay, base)
            g["gfeat_part"] = self.parts[i].f.view(M, FEAT)
            assert self.parts[i].written(), ("gfeat_parts", i)
            for k in GEN_GRADS:
                assert self.gen_grads[i][k].written(), ("gradient", i, k)
                g["d" + k] = self.gen_grads[i][k].f.view(self.d["nets"][i][k].shape)
            gens.append(g)
        assert self.scratch.only_written(regions, free), "scratch"
        lay, end = R.deform_scratch_layout(M)
        assert self.scratch_deform.only_written(_regions(lay), [(end, self.scratch_deform.n - end)]), "scratch_deform"
        assert self.gfeat_sum.written(), "gfeat_sum"
        g = self.scratch_deform.views({k: v for k, v in lay.items() if k.startswith("g")})
        g["gfeat_sum"] = self.gfeat_sum.f.view(M, FEAT)
        for i in range(5):
            assert self.def_grads["W"][i].written() and self.def_grads["b"][i].written(), ("deform gradient", i)
            g[f"dW{i}"] = self.def_grads["W"][i].f.view(self.d["deform"]["W"][i].shape)
            g[f"db{i}"] = self.def_grads["b"][i].f.view(-1)
        return gens, g


def _statements(p, dt, got_fw, y, gy, exact, bwd_acts):
    """The forward and backward statements of Pass p in dtype dt on the GPU; the backward on the kernel's own saved tensors."""
    c = R.cast(p.c, dt, "cuda")
    fw = R.generators_forward_ref(c["nets"], c["feat"], c["cond"], c["film"]) + [R.deform_forward_ref(c["deform"], c["feat"], c["cond"])]
    nets_b = [dict(net, act=a) for net, a in zip(c["nets"], bwd_acts)] if bwd_acts else c["nets"]
    saved = [{k: v.to(dt) for k, v in g.items()} for g in got_fw]
    cf = c["film"]["cond"] if c["film"] else c["cond"]
    gens = R.generators_backward_ref(nets_b, c["feat"], cf, saved[:p.n], [t.to(dt) for t in y], [t.to(dt) for t in gy[:p.n]], c["film"], exact=exact)
    parts = [(o["gfeat_part"][0], o["gfeat_part"][1]) for o in gens]
    deform = R.deform_backward_ref(c["deform"], c["feat"], c["cond"], saved[p.n], gy[p.n].to(dt), parts, exact=exact)
    return fw, gens, deform


def _step_statements(p, dt, got_fw, got_gens, got_def):
    """The single-step statements in dtype dt on the kernel's own stored tensors: per network forward, per generator backward, the
    deformation network's backward."""
    c = R.cast(p.c, dt, "cuda")
    to = lambda g: {k: v.to(dt) for k, v in g.items()}  # noqa: E731
    fw, gens = [to(g) for g in got_fw], [to(g) for g in got_gens]
    s_fw = R.generators_forward_steps(c["nets"], fw[:p.n], c["film"]) + [R.deform_forward_steps(c["deform"], fw[p.n])]
    s_gens = R.generators_backward_steps(c["nets"], c["feat"], c["cond"], fw[:p.n], gens, c["film"])
    s_def = R.deform_backward_steps(c["deform"], c["feat"], c["cond"], fw[p.n], to(got_def), [g["gfeat_part"] for g in gens])
    return s_fw, s_gens, s_def


def _run_case(tag, kind, M, n, Mf=None, one_sided=False):
    """Forward and backward of one case and kind, every tensor compared; returns the Pass and what it wrote."""
    exact = kind != "randn"
    bwd_acts = R.EXACT_ACTS[n] if kind == "lin" else None
    c = R.build_case(kind, M, n, Mf, one_sided)
    p = Pass(c, bwd_acts)
    assert p.forward() == OK, p.L.gsvc_last_error()
    got_fw = p.forward_got()
    y = [p.y[i].f.view(M, -1).clone() if kind == "randn" else p.d["ys"][i] for i in range(n)]
    gy = p.d["gys"]
    assert p.backward(y, gy) == OK, p.L.gsvc_last_error()
    got_gens, got_def = p.backward_got()
    fw64, gens64, def64 = _statements(p, f64, got_fw, y, gy, exact, bwd_acts)
    fw32, gens32, def32 = (None, [None] * n, None) if exact else _statements(p, f32, got_fw, y, gy, exact, bwd_acts)
    for i in range(n + 1):
        who = f"{tag} {kind} " + (f"gen{i}" if i < n else "deform")
        _compare(who + " fwd", got_fw[i], fw64[i], None if exact else fw32[i])
        _compare(who + " bwd", got_gens[i] if i < n else got_def, gens64[i] if i < n else def64, None if exact else (gens32[i] if i < n else def32))
    if not exact:      # every stored tensor against its own step on the stored tensors that step read: the rule with L = 1
        s64, s32 = _step_statements(p, f64, got_fw, got_gens, got_def), _step_statements(p, f32, got_fw, got_gens, got_def)
        for i in range(n + 1):
            who = f"{tag} {kind} " + (f"gen{i}" if i < n else "deform")
            _compare(who + " fwd step", got_fw[i], s64[0][i], s32[0][i])
            _compare(who + " bwd step", got_gens[i] if i < n else got_def, s64[1][i] if i < n else s64[2], s32[1][i] if i < n else s32[2])
    if kind in ("one", "one_cond") and not Mf:
        for i in range(n):
            _single(f"{tag} {kind} y{i}", got_fw[i]["y"], 18.0 if kind == "one" else 8.0)
        _single(f"{tag} {kind} deform y", got_fw[n]["y"], 8.0)
    if Mf:      # a FiLM row with neither side: the sums are +0, bit for bit
        none = ((p.film["src_a"] < 0) & (p.film["src_b"] < 0)).nonzero().view(-1)
        for i in range(n):
            for k in ("ggamma", "gbeta"):
                assert bool((got_gens[i][k].view(torch.int32)[none] == 0).all()), (tag, kind, i, k, "a FiLM row with neither side is not +0")
    return p, got_fw, got_gens, got_def, (y, gy)


# ------------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("M,n,exact", R.GEN_CASES, ids=lambda v: str(v))
def test_generate_all(M, n, exact):
    """One FiLM row per chain row: row counts around a 16-row block, one and two generators, grids that are no multiple of the network
    count (M = 150), the mid size and the second round of the persistent loop (M = 11003 with three networks, 32785 with one)."""
    for kind in ("randn", "one", "one_cond") + (("lin",) if exact else ()):
        _run_case(f"M{M} n{n}", kind, M, n)


@pytest.mark.parametrize("M,Mf,one_sided,exact", R.SHARED_CASES, ids=lambda v: str(v))
def test_generate_all_shared_film(M, Mf, one_sided, exact):
    """Shared FiLM rows (three generators): rows with both sides, only a, only b and neither, shuffled maps, Mf = 1, and the second
    round over FiLM blocks.  The chain-row outputs equal, bit for bit, those of the unshared run on cond_film[row_of]."""
    tag = f"M{M} Mf{Mf}"
    if Mf > 1 and not one_sided:
        both, only_a, only_b, neither = R.map_kinds(*R.film_map(M, Mf, 0)[1:])
        assert min(both, only_a, only_b, neither) > 0, (tag, both, only_a, only_b, neither)
    for kind in ("randn", "one") + (("lin",) if exact else ()):
        p, fw, gens, deform, (y, gy) = _run_case(tag, kind, M, 3, Mf, one_sided)
        if kind != "randn":
            continue
        c = dict(p.c, film=None)
        q = Pass(c)
        assert q.forward() == OK and q.backward(y, gy) == OK
        fw_u, (gens_u, deform_u) = q.forward_got(), q.backward_got()
        for i in range(3):
            for k in ("a1", "h", "x3", "y"):
                assert torch.equal(fw[i][k], fw_u[i][k]), (tag, i, k, "shared and unshared runs differ")
            for k in ("go", "gh", "gz1", "gfeat_part"):      # (the weight gradients' row split follows the batch of products: not bit-equal)
                assert torch.equal(gens[i][k], gens_u[i][k]), (tag, i, k, "shared and unshared runs differ")
            assert torch.equal(fw[i]["gamma"][p.film["row_of"].long()], fw_u[i]["gamma"]), (tag, i, "gamma")
        for k in ("g1", "g2", "g3", "g4", "gfeat_sum"):
            assert torch.equal(deform[k], deform_u[k]), (tag, "deform", k)


@pytest.mark.parametrize("M", R.INFERENCE_M)
def test_inference_forward(M):
    """keep_for_backward = 0, shared and not: y equals the keeping run's bit for bit; saved[i] holds gamma / beta (the deformation
    network: a2) at its start and every sentinel behind them survives."""
    for Mf in (None, R.INFERENCE_SHARED[M]):
        p = Pass(R.build_case("randn", M, 3, Mf))
        assert p.forward(keep=1) == OK
        kept = [{k: v.clone() for k, v in g.items()} for g in p.forward_got()]
        p.new_forward_buffers()
        assert p.forward(keep=0) == OK
        got = p.forward_got(inference=True)
        for i in range(4):
            for k in got[i]:
                assert torch.equal(got[i][k], kept[i][k]), (M, Mf, i, k, "the inference run differs from the keeping run")


def _quant_call(nets, X, dq, z_off=0, in_dim=R.Q_IN):
    """The two quant_step entries on sentinel buffers; ({z, a, q} per network, {dz} per network, dX, buffers, return codes)."""
    lb, L, st = _lib()
    M = X.shape[0]
    d = R.cast(nets, f32, "cuda")
    arr = (lb.QuantStepNetC * 3)()
    for i, n in enumerate(d):
        arr[i].W1, arr[i].b1, arr[i].W2, arr[i].b2 = (n[k].data_ptr() for k in ("W1", "b1", "W2", "b2"))
    Xd, dqd = X.cuda(), [None if t is None else t.cuda() for t in dq]
    z, a, q = ([Buf(M * w + 4) for _ in range(3)] for w in (R.Q_HID, R.Q_HID, 1))
    dz, dX = [Buf(M * R.Q_HID) for _ in range(3)], Buf(M * R.Q_IN)
    bufs = z + a + q + dz + [dX]
    rc_f = L.gsvc_quant_step_nets_forward(arr, Xd.data_ptr(), M, in_dim, R.Q_HID, _ptrs([b.ptr + 4 * z_off for b in z]), _ptrs([b.ptr for b in a]),
                                          _ptrs([b.ptr for b in q]), st)
    torch.cuda.synchronize()
    if rc_f != OK:
        return None, None, None, bufs, (rc_f, None)
    rc_b = L.gsvc_quant_step_nets_backward(arr, _ptrs([b.ptr for b in z]), _ptrs([None if t is None else t.data_ptr() for t in dqd]), M, in_dim,
                                           R.Q_HID, _ptrs([b.ptr for b in dz]), dX.ptr, st)
    torch.cuda.synchronize()
    fw = []
    for i in range(3):
        assert z[i].only_written([(0, M * R.Q_HID)]) and a[i].only_written([(0, M * R.Q_HID)]) and q[i].only_written([(0, M)]), ("quant forward", i)
        assert dz[i].written(), ("dz", i)
        fw.append({"z": z[i].f[:M * R.Q_HID].view(M, R.Q_HID), "a": a[i].f[:M * R.Q_HID].view(M, R.Q_HID), "q": q[i].f[:M]})
    assert dX.written(), "dX"
    return fw, [{"dz": b.f.view(M, R.Q_HID)} for b in dz], dX.f.view(M, R.Q_IN), bufs, (rc_f, rc_b)


@pytest.mark.parametrize("M", R.QUANT_M)
def test_quant_step_nets(M):
    """The three quant_step networks in one launch each way: z, a, q forward; dz, dX backward on the forward's own z; once with
    dq[1] = NULL (zeros).  M = 32785: the second round of the persistent loop."""
    for kind, drop in (("randn", False), ("randn", True), ("lin", False), ("lin", True), ("one", False)):
        nets = R.make_quant(kind, 50 + M)
        X, dq = R.make_quant_rows(kind, M, 60 + M)
        if drop:
            dq[1] = None
        fw, bw, dX, _, rc = _quant_call(nets, X, dq)
        assert rc == (OK, OK)
        tag = f"quant M{M} {kind}{' dq1=NULL' if drop else ''}"
        ref = {}
        for dt in (f64,) if kind != "randn" else (f64, f32):
            n_, X_, dq_ = R.cast(nets, dt, "cuda"), X.to("cuda", dt), [None if t is None else t.to("cuda", dt) for t in dq]
            r_fw = R.quant_nets_forward_ref(n_, X_)
            r_bw, r_dX = R.quant_nets_backward_ref(n_, [g["z"].to(dt) for g in fw], dq_, exact=kind != "randn")
            ref[dt] = (r_fw, r_bw, r_dX)
        for i in range(3):
            _compare(f"{tag} net{i} fwd", fw[i], ref[f64][0][i], ref[f32][0][i] if kind == "randn" else None)
            _compare(f"{tag} net{i} bwd", bw[i], ref[f64][1][i], ref[f32][1][i] if kind == "randn" else None)
        _compare(tag, {"dX": dX}, {"dX": ref[f64][2]}, {"dX": ref[f32][2]} if kind == "randn" else None)
        if kind == "randn":      # a, q and dX against their own steps on the stored z, a and dz
            st = {dt: R.quant_nets_steps(R.cast(nets, dt, "cuda"), [{k: v.to(dt) for k, v in g.items()} for g in fw],
                                         [{k: v.to(dt) for k, v in g.items()} for g in bw]) for dt in (f64, f32)}
            for i in range(3):
                _compare(f"{tag} net{i} fwd step", fw[i], st[f64][0][i], st[f32][0][i])
            _compare(tag + " step", {"dX": dX}, {"dX": st[f64][1]}, {"dX": st[f32][1]})
        if drop:
            assert bool((bw[1]["dz"] == 0).all()), tag
        if kind == "one":
            for i in range(3):
                want = torch.zeros(M, device="cuda")
                want[M - 1] = 8.0
                assert torch.equal(fw[i]["q"], want), tag
            want = torch.zeros(M, R.Q_IN, device="cuda")
            want[M - 1, R.Q_IN - 1] = 3.0
            assert torch.equal(dX, want), tag


# ------------------------------------------------------------------------------------------------------------ refusals
def test_generate_all_refusals():
    """Every refused call returns its documented code and leaves every sentinel buffer untouched; M = 0 is GSVC_OK with nothing written.
    (The 2 GiB row-map refusal is not tested: it would need dummy pointers that a wrong check would dereference.)"""
    M, n = 17, 3
    p = Pass(R.build_case("randn", M, n))
    assert p.forward() == OK
    y = [p.y[i].f.view(M, -1).clone() for i in range(n)]
    gy = p.d["gys"]
    side = torch.cuda.Stream()

    def refused(code, what, fwd=True, bwd=True, wgrad_stream=None, **over):
        q = Pass(p.c)
        if fwd:
            assert q.forward(**over) == code, (what, "forward")
            assert all(b.untouched() for b in q.saved + q.y), (what, "forward wrote")
        if bwd:
            q.saved = p.saved      # a valid forward's saved tensors
            assert q.backward(y, gy, wgrad_stream=wgrad_stream, **over) == code, (what, "backward")
            assert all(b.untouched() for b in q.backward_buffers()), (what, "backward wrote")
        return q

    def nets_with(**fields):
        arr = (p.lb.GeneratorNetC * 3)()
        for i in range(3):
            C.memmove(C.byref(arr[i]), C.byref(p.nets[i]), C.sizeof(p.lb.GeneratorNetC))
        for k, v in fields.items():
            setattr(arr[0], k, v)
        return arr

    refused(E_UNSUPPORTED, "hidden_dim 96", nets=nets_with(hidden_dim=96))
    refused(E_UNSUPPORTED, "out_dim 20", nets=nets_with(out_dim=20))
    refused(E_UNSUPPORTED, "out_act 3", nets=nets_with(out_act=3))
    refused(E_INVALID, "n_nets 0", n=0)
    refused(E_INVALID, "n_nets 4", n=4)
    refused(E_INVALID, "M < 0", M=-1)
    refused(E_INVALID, "feat off alignment", feat=p.d["feat"].data_ptr() + 4)
    refused(E_INVALID, "NULL weight pointer", nets=nets_with(W2=None))
    q = Pass(p.c)
    refused(E_INVALID, "gfeat_parts[0] == gfeat_parts[1]", fwd=False, parts=_ptrs([q.parts[0].ptr, q.parts[0].ptr, q.parts[2].ptr]))
    assert q.parts[0].untouched()
    refused(E_INVALID, "gfeat_parts[1] == gfeat_sum", fwd=False, parts=_ptrs([q.parts[0].ptr, q.gfeat_sum.ptr, q.parts[2].ptr]), gfeat_sum=q.gfeat_sum.ptr)
    assert q.parts[0].untouched() and q.gfeat_sum.untouched()
    refused(E_INVALID, "scratch overlapping scratch_deform with a wgrad_stream", fwd=False, wgrad_stream=C.c_void_p(side.cuda_stream),
            scratch=q.scratch.ptr, scratch_deform=q.scratch.ptr + 64)
    assert q.scratch.untouched()
    refused(OK, "M = 0", M=0)


def test_quant_step_nets_refusals():
    """in_dim = 191 and a z one float off alignment: GSVC_E_UNSUPPORTED, nothing written."""
    M = 17
    nets = R.make_quant("randn", 1)
    X, dq = R.make_quant_rows("randn", M, 2)
    for what, kw in (("in_dim 191", dict(in_dim=191)), ("misaligned z", dict(z_off=1))):
        _, _, _, bufs, rc = _quant_call(nets, X, dq, **kw)
        assert rc[0] == E_UNSUPPORTED, what
        assert all(b.untouched() for b in bufs), what
