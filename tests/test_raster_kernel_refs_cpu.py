"""The NumPy statements of tests/_raster_kernel_refs.py pinned on the CPU (no GPU): the two forms against each other in float64, the
float64 run against the C oracle and against the dense float64 autograd statement, preprocess_ref in float32 against the oracle's
``geom`` bit for bit, and the borderline share of every scene tests/test_raster_kernels_gpu.py uses."""
import functools

import numpy as np
import pytest
import torch

from gsvc_amd import synthetic
from tests import _raster_kernel_refs as K
from tests._dense_raster import dense_render

BG = (0.3, 0.1, 0.6)


@functools.lru_cache(maxsize=None)
def _forward(name):
    import oracle
    oracle.build()
    sc = K.scene(name)
    st = dict(sc["settings"], bg=BG)
    fw = K.oracle_forward(oracle, sc, bg=BG)
    r64, r32, border = K.forward_refs(fw.geom, sc["opacities"], sc["colors"], fw.tile_ranges, fw.point_list, st, fw.borderline)
    return sc, st, fw, r64, r32, border


def _lists(sc, st, fw):
    return fw.geom, sc["opacities"], sc["colors"], fw.tile_ranges, fw.point_list, st


def _dL(shape, border, seed=5):
    dL = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    dL[..., border] = 0
    return dL


def _inputs(sc, fw):
    return dict(means3D=sc["means3D"], scales=sc["scales"], rotations=sc["rotations"], opacities=sc["opacities"], radii=fw.radii)


@pytest.mark.parametrize("name", ["R300", "R400", "S65", "S5c", "B"])
def test_literal_and_polynomial_forms_agree_in_float64(oracle_lib, name):
    """Image, rows and the shifted moments: 1e-12 of each element's scale (positive definite conics: what the polynomial serves).
    R400 (half-pixel-wide Gaussians of up to 12 px, seen from tiles away) is where the shift `U^2 m0 - 2 U mx + mxx` cancels most:
    its terms add up to sum |h| (|U| + |x|)^2 and leave sum |h| dx^2, so float64 itself leaves 1.3e-12 of scale there.  Its bar
    for the six moments is the cancellation's own: 1e-12 of scale + 16 eps64 of what the shift adds up (16: a pairwise sum of 256
    pixels, 8 roundings, and the 8 operations of the shift and the division by o)."""
    sc, st, fw, r64, _, border = _forward(name)
    args = _lists(sc, st, fw)
    poly = K.blend_ref(*args, np.float64, "poly", decisions=r64["decisions"])
    assert K.rule_error(poly["image"], r64["image"], r64["image_scale"]) < 1e-12
    assert np.abs(poly["final_T"] - r64["final_T"]).max() < 1e-12
    for flags in (0, K.F_CLAMP_STOP):
        a2 = args[:5] + (dict(st, flags=flags),)
        dL = _dL((3, st["H"], st["W"]), border)
        lit, mags = K.blend_bwd_rows_ref(*a2, r64["final_T"], r64["decisions"], dL, np.float64, "literal")
        added = np.zeros((lit.shape[0], 6))
        pol, _ = K.blend_bwd_rows_ref(*a2, r64["final_T"], r64["decisions"], dL, np.float64, "poly", shift_mags=added)
        assert np.abs(lit).max() > 0
        if name != "R400":
            assert K.rule_error(pol, lit, mags) < 1e-12
        tol = 1e-12 * mags
        tol[:, :6] += 16 * np.finfo(np.float64).eps * added
        assert np.all(np.abs(pol - lit) <= tol), float((np.abs(pol - lit) / np.maximum(tol, 1e-300)).max())


@pytest.mark.parametrize("name", ["R300", "R400", "L300", "S129", "S64c", "B"])
def test_float64_forward_is_the_oracles_at_float32_level(oracle_lib, name):
    sc, st, fw, r64, r32, border = _forward(name)
    ok = ~border
    assert np.array_equal(fw.n_contrib[ok], r64["n_contrib"][ok])
    e32 = K.rule_error(r32["literal"]["image"], r64["image"], r64["image_scale"], keep=np.broadcast_to(ok, (3,) + ok.shape))
    e_or = K.rule_error(fw.image, r64["image"], r64["image_scale"], keep=np.broadcast_to(ok, (3,) + ok.shape))
    assert K.within_rule(e_or, e32), (e_or, e32)
    eT32 = np.abs(r32["literal"]["final_T"] - r64["final_T"])[ok].max()
    assert K.within_rule(np.abs(fw.final_T - r64["final_T"])[ok].max(), eT32)


@pytest.mark.parametrize("name,flags", [("R300", 0), ("R400", K.F_CLAMP_STOP), ("L300", 0), ("S5c", K.F_CLAMP_STOP), ("B", 0)])
def test_float64_rows_summed_reproduce_the_six_oracle_gradients(oracle_lib, name, flags):
    sc, st, fw, r64, r32, border = _forward(name)
    st = dict(st, flags=int(st.get("flags", 0)) | flags)
    s = dict(sc["settings"], flags=st["flags"])
    args = _lists(sc, st, fw)
    dL = _dL((3, st["H"], st["W"]), border)
    rb = oracle_lib.raster_backward(K.oracle_settings(oracle_lib, s, bg=BG), sc["means3D"], sc["colors"], sc["opacities"], sc["scales"],
                                    sc["rotations"], fw, dL)
    P = sc["means3D"].shape[0]
    rows, mags = K.blend_bwd_rows_ref(*args, r64["final_T"], r64["decisions"], dL, np.float64, "literal")
    rows32, _ = K.blend_bwd_rows_ref(*args, r32["literal"]["final_T"], r64["decisions"], dL, np.float32, "literal")
    inp = _inputs(sc, fw)
    g = K.gaussian_bwd_ref(K.sum_rows_per_gaussian(rows, fw.point_list, P), inp, st, np.float64)
    gm = K.gaussian_bwd_ref(K.sum_rows_per_gaussian(mags, fw.point_list, P), inp, st, np.float64, mag=True)
    g32 = K.gaussian_bwd_ref(K.sum_rows_per_gaussian(rows32, fw.point_list, P, np.float32), inp, st, np.float32)
    for k in K.GRADS:
        e_or, e32 = K.rule_error(getattr(rb, k), g[k], gm[k]), K.rule_error(g32[k], g[k], gm[k])
        assert np.abs(g[k]).max() > 0
        assert K.within_rule(e_or, e32), (k, e_or, e32)


@pytest.mark.parametrize("name", ["R400", "B"])
def test_cov3d_branch_of_gaussian_bwd_ref_against_the_oracle(oracle_lib, name):
    """The oracle has no covariance source, so the branch is held to it through the chain rule: with cov3D = R S^2 R^T (float32, the
    bits the scale / rotation call forms) the other five gradients are the scale / rotation call's, dL/dscales and dL/drotations
    are zeros, and dL/dcov3D per stored number, taken through cov3D(s, q) by float64 autograd, gives the oracle's dL/dscales and
    dL/drotations — all at float32 level (the rule, e32 = the float32 run of the scale / rotation branch)."""
    from tests._dense_raster import quat_to_rot
    sc, st, fw, r64, r32, border = _forward(name)
    args = _lists(sc, st, fw)
    dL = _dL((3, st["H"], st["W"]), border)
    rb = oracle_lib.raster_backward(K.oracle_settings(oracle_lib, sc["settings"], bg=BG), sc["means3D"], sc["colors"], sc["opacities"],
                                    sc["scales"], sc["rotations"], fw, dL)
    P = sc["means3D"].shape[0]
    rows, mags = K.blend_bwd_rows_ref(*args, r64["final_T"], r64["decisions"], dL, np.float64, "literal")
    rows32, _ = K.blend_bwd_rows_ref(*args, r32["literal"]["final_T"], r64["decisions"], dL, np.float32, "literal")
    tot, totm = K.sum_rows_per_gaussian(rows, fw.point_list, P), K.sum_rows_per_gaussian(mags, fw.point_list, P)
    inp = _inputs(sc, fw)
    g, gm = K.gaussian_bwd_ref(tot, inp, st, np.float64), K.gaussian_bwd_ref(totm, inp, st, np.float64, mag=True)
    g32 = K.gaussian_bwd_ref(K.sum_rows_per_gaussian(rows32, fw.point_list, P, np.float32), inp, st, np.float32)
    cov = K.cov3d_ref(sc["scales"], sc["rotations"], st, np.float32)
    inp_c = dict(means3D=sc["means3D"], opacities=sc["opacities"], radii=fw.radii, cov3D=cov)
    c, cm = K.gaussian_bwd_ref(tot, inp_c, st, np.float64), K.gaussian_bwd_ref(totm, inp_c, st, np.float64, mag=True)
    assert c["cov3D"].shape == (P, 6) and np.abs(c["cov3D"]).max() > 0 and np.all(cm["cov3D"] >= np.abs(c["cov3D"]))
    assert not np.any(c["scales"]) and not np.any(c["rotations"]) and not np.any(cm["scales"]) and not np.any(cm["rotations"])
    e32 = {k: K.rule_error(g32[k], g[k], gm[k]) for k in K.GRADS}
    for k in ("means2D", "means3D", "colors", "opacities"):
        assert K.within_rule(K.rule_error(c[k], g[k], gm[k]), e32[k]), k
    s_t = torch.tensor(sc["scales"].astype(np.float64), requires_grad=True)
    q_t = torch.tensor(sc["rotations"].astype(np.float64), requires_grad=True)
    Lm = quat_to_rot(q_t) * (s_t * float(st["scale_modifier"]))[:, None, :]
    S3 = Lm @ Lm.transpose(1, 2)
    stored = torch.stack([S3[:, 0, 0], S3[:, 0, 1], S3[:, 0, 2], S3[:, 1, 1], S3[:, 1, 2], S3[:, 2, 2]], dim=1)
    (stored * torch.tensor(c["cov3D"])).sum().backward()
    for k, t in (("scales", s_t), ("rotations", q_t)):
        chained = t.grad.numpy()
        assert np.abs(chained).max() > 0
        assert K.within_rule(K.rule_error(chained, g[k], gm[k]), e32[k]), (k, K.rule_error(chained, g[k], gm[k]), e32[k])
        assert K.within_rule(K.rule_error(getattr(rb, k), chained, gm[k]), e32[k]), k


@pytest.mark.parametrize("P,seed", [(40, 0), (30, 3)])
def test_dense_float64_autograd_reproduces_the_float64_chain(oracle_lib, P, seed):
    """tests/_dense_raster.py differentiated by autograd, at the two tiny sizes tests/test_oracle_raster.py uses: the same six
    gradients as preprocess_ref -> blend_ref -> blend_bwd_rows_ref -> gaussian_bwd_ref, everything in float64 from the inputs."""
    sc = synthetic.raster_scene(P, H=40, W=56, T=32, seed=seed, window_frames=8, sigma_px=(1.0, 5.0))
    s = dict(sc["settings"], bg=BG)
    for k in ("scale", "x_min", "y_min"):          # the settings as the C ABI carries them (binary32), for both statements
        s[k] = float(np.float32(s[k]))
    s["bg"], s["low_pass"] = tuple(float(np.float32(b)) for b in BG), float(np.float32(0.3))
    fw = K.oracle_forward(oracle_lib, sc, bg=BG)
    pre = K.preprocess_ref(sc["means3D"], sc["scales"], sc["rotations"], s, np.float64)
    geom = np.stack([pre[k] for k in ("u", "v", "depth", "A", "B", "C")], axis=1)
    args = (geom, sc["opacities"], sc["colors"], fw.tile_ranges, fw.point_list, s)
    r64 = K.blend_ref(*args, np.float64, "literal")
    border = r64["borderline"] | (fw.borderline != 0)
    dL = _dL((3, s["H"], s["W"]), border)
    rows, mags = K.blend_bwd_rows_ref(*args, r64["final_T"], r64["decisions"], dL, np.float64, "literal")
    inp = _inputs(sc, fw)
    g = K.gaussian_bwd_ref(K.sum_rows_per_gaussian(rows, fw.point_list, P), inp, s, np.float64)
    gm = K.gaussian_bwd_ref(K.sum_rows_per_gaussian(mags, fw.point_list, P), inp, s, np.float64, mag=True)

    t = {k: torch.tensor(sc[k].astype(np.float64), requires_grad=True) for k in ("means3D", "colors", "opacities", "scales", "rotations")}
    delta = torch.zeros(P, 2, dtype=torch.float64, requires_grad=True)
    img = dense_render(s, t["means3D"], t["colors"], t["opacities"].view(-1), t["scales"], t["rotations"], fw.radii, uv_delta=delta)
    assert np.abs(img.detach().numpy() - r64["image"])[:, ~border].max() < 1e-12
    (img * torch.tensor(dL.astype(np.float64))).sum().backward()
    dense = {k: t[k].grad.numpy() for k in t}
    dense["means2D"] = np.concatenate([delta.grad.numpy() * np.array([0.5 * s["W"], 0.5 * s["H"]]), np.zeros((P, 1))], axis=1)
    # the oracle's formulas (and so gaussian_bwd_ref) divide by det^2 + 1e-7 where the derivative has det^2: the covariance's
    # gradients of Gaussian i are smaller by the factor 1 / (1 + 1e-7 / det_i^2) than autograd's
    reg = 1e-7 / pre["det"] ** 2
    for k in K.GRADS:
        assert np.abs(g[k]).max() > 0
        tol = 1e-9 + (reg[:, None] if k in ("scales", "rotations") else 0.0)
        err = np.abs(dense[k].reshape(g[k].shape) - g[k])
        assert np.all(err <= tol * gm[k]), (k, float((err / np.maximum(gm[k], 1e-300)).max()))


@pytest.mark.parametrize("name", ["R400", "L300", "B"])
def test_preprocess_ref_in_float32_gives_the_oracles_geom(oracle_lib, name):
    sc, st, fw, _, _, _ = _forward(name)
    pre = K.preprocess_ref(sc["means3D"], sc["scales"], sc["rotations"], st, np.float32)
    live = fw.radii > 0
    assert live.sum() > 10
    for col, k in enumerate(("u", "v", "depth", "A", "B", "C")):
        assert pre[k].dtype == np.float32
        assert np.array_equal(pre[k][live].view(np.uint32), fw.geom[live, col].view(np.uint32)), k


@pytest.mark.parametrize("name", sorted(K.SCENES))
def test_borderline_share_of_every_gpu_scene_is_under_its_cap(oracle_lib, name):
    """A condition on the scenes, not a measurement: the share of pixels the references alone call borderline (a float64 decision
    inside the oracle's margins, a float32 form deciding differently, the oracle's mark) stays under the caps
    tests/test_raster_gpu.py uses: 5e-4, and 5e-3 for the stacked single-tile scenes."""
    _, _, _, r64, _, border = _forward(name)
    assert border.mean() <= K.borderline_cap(name), (name, border.mean())
    if name.startswith("S"):
        n = int(name[1:].rstrip("c"))
        last = r64["n_contrib"][:16, :16]
        if name.endswith("c"):
            assert any(c.any() for _, c in r64["decisions"].values())     # the 0.99 clamp is reached
            assert n < 63 or last.min() < n         # the T < 1e-4 stop leaves entries behind the last contributor
        else:
            for qy in (0, 8):                        # nothing stops early, and every quadrant holds all n entries
                for qx in (0, 8):
                    assert last[qy:qy + 8, qx:qx + 8].max() == n, (qy, qx)


@pytest.mark.parametrize("name", ["R300", "R400", "R600", "L300", "B"])
def test_print_the_gap_the_global_maximum_rule_leaves(oracle_lib, name, capsys):
    """Per gradient, the smallest per-Gaussian scale over the largest: a Gaussian at that ratio can be wrong in every digit under
    `max |got - ref| / max |ref| < 1e-4` as soon as the ratio is below 1e-4 (DESIGN.md section 4h lists the figures)."""
    sc, st, fw, r64, _, border = _forward(name)
    dL = _dL((3, st["H"], st["W"]), border)
    _, mags = K.blend_bwd_rows_ref(*_lists(sc, st, fw), r64["final_T"], r64["decisions"], dL, np.float64, "literal")
    P = sc["means3D"].shape[0]
    gm = K.gaussian_bwd_ref(K.sum_rows_per_gaussian(mags, fw.point_list, P), _inputs(sc, fw), st, np.float64, mag=True)
    with capsys.disabled():
        for k in K.GRADS:
            per = gm[k].max(axis=1)
            ratio = per[per > 0].min() / per.max()
            print(f"SCALE_RATIO {name} {k} {ratio:.2e}")
            assert 0 < ratio <= 1
