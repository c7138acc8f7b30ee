"""The source block of Born modelling and of the exact adjoint on the GPU (-m gpu): sepfwi_born_src, sepfwi_adjoint_exact_src and the
keywords of fwi_ops.born / born_adjoint / gauss_newton / backward, against the CPU oracle alone.  The wavefield is exactly linear in the
source time function, so J_s ds is the oracle's own gathers with stf = ds (tests/stf_ref.py js_ref, licensed on the CPU by
tests/test_stf_reference.py), J_m v is tests/born_ref.py, and the adjoint side is defined by them: <J u, w> = <u, J^T w> in float64.

Problems: tests/problems.make_problem at its defaults (44 x 60 physical, nPml 10, 240 steps, 2 shots); for the unit spikes also the same
problem with the fibre on the source's row (rec_z = src_z), where a spike at step nSteps-2 reaches the channels within the record.

Tolerances, none new (tests/test_gpu_exact_adjoint.py, tests/fuzz_common.py):
    scalars      |got - ref| <= 1e-3 scale + 3 |ref_nvfma - ref|     (exact_adjoint_ref.held; scale |ref|, or the product of the two norms
                                                                      of a dot product of unrelated vectors)
    gathers      1e-4 of the component's maximum and rel-L2 1e-4, plus 3 x the two oracle builds' difference
    misfit       1e-4 of f(stf)
Every comparison prints its deviation before it asserts; profiles/r16_source_adjoint.txt holds the figures measured on the MI355X.
Every test fails on the parent commit: the two entry points and the keywords do not exist there."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_adjoint_ref as X
import fuzz_common as FC
import problems as P
import stf_ref as S
from conftest import ROOT
from exact_adjoint_ref import WEIGHTS, cuda, held
from stf_ref import exact_src
from fuzz_common import write_para

pytestmark = pytest.mark.gpu
COMPS = X.COMPS


# ---- the reference side ----------------------------------------------------------------------------------------------------------------
def born_src(pb, fn, **kw):
    """stf_ref.born_src -> {component: (nshots, nrec, nSteps)}"""
    return stack(S.born_src(pb, fn, **kw))


def stack(per_shot):
    return {c: np.stack([np.asarray(s[c], np.float64) for s in per_shot]) for c in COMPS}


def js(lib, pb, ds, para=None, model="lame_init"):
    """js_ref -> {component: (nshots, nrec, nSteps) float64}"""
    return stack(S.js_ref(lib, [t.numpy() for t in pb[model]], ds, pb["Shot_ids"].numpy(), para or pb["para"], pb["survey"]))


def add(a, b):
    return {c: np.asarray(a[c], np.float64) + np.asarray(b[c], np.float64) for c in COMPS}


def shot(a, i):
    return {c: x[i:i + 1] for c, x in a.items()}


def norm(a, weights=(1.0, 0.0, 0.0)):
    return float(np.sqrt(X.data_dot(a, a, weights)))


def gathers_held(got, ref, alt, what):
    """per shot and component: max deviation <= 1e-4 of the component's maximum, rel-L2 <= 1e-4, each plus 3 x the two builds'"""
    for c in COMPS:
        for i in range(ref[c].shape[0]):
            g, r, a = got[c][i], ref[c][i], alt[c][i]
            top = float(np.abs(r).max())
            assert top > 0, (what, c, i)
            dmax, dl2 = float(np.abs(g - r).max()), FC.d64(g, r)
            print("source adjoint %s, shot %d %s: max deviation %.2e of the peak, rel-L2 %.2e (the two oracle builds %.2e, %.2e)"
                  % (what, i, c, dmax / top, dl2 / FC.l2(r), float(np.abs(a - r).max()) / top, FC.d64(a, r) / FC.l2(r)))
            assert dmax <= FC.GATHER_TOL * top + FC.YARD * float(np.abs(a - r).max()), (what, c, i)
            assert FC.array_held(g, r, a, FC.GATHER_TOL), (what, c, i)


@pytest.fixture(scope="module")
def prob(oracle, oracle_nvfma, hip_ops, tmp_path_factory):
    """The default problem, one v on Omega, two source perturbations, and J_m v, J_s ds of both oracle builds: computed once, left unchanged"""
    pb = P.make_problem(str(tmp_path_factory.mktemp("source_adjoint")))
    stf = pb["Stf"].numpy()
    vs = [X.smooth_v(pb, 3), X.white_v(pb, 5)]
    dss = [S.draw_ds(0, stf, S.DS_SCALE), S.draw_ds(1, stf, S.DS_SCALE)]
    ref = dict(jv=[X.jv_ref(oracle, pb, v) for v in vs], js=[js(oracle, pb, d) for d in dss])
    alt = dict(jv=[X.jv_ref(oracle_nvfma, pb, v) for v in vs], js=[js(oracle_nvfma, pb, d) for d in dss])
    return pb, vs, dss, ref, alt


# ---- 1. Born ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["default", "joint", "gauge3"])
def test_born_of_a_source_perturbation_is_the_forward_operator(oracle, oracle_nvfma, hip_ops, prob, kind):
    """1: sepfwi_born_src with v = NULL and ds gives the oracle's gathers of stf = ds, per shot, for ett, vx and vz; with a joint-weight
    parameter file; with a gauge length of 3 cells."""
    pb, vs, dss, ref, alt = prob
    hip_ops.release()
    keys = dict(joint=dict(misfit_w_ett=1.0, misfit_w_vx=0.5, misfit_w_vz=0.25), gauge3=dict(das_gauge_length=3 * pb["para"]["dx"])).get(kind, {})
    fn, para = write_para(pb, "born_" + kind, **keys)
    r, a = (ref["js"][0], alt["js"][0]) if kind != "gauge3" else (js(oracle, pb, dss[0], para), js(oracle_nvfma, pb, dss[0], para))
    gathers_held(born_src(pb, fn, ds=dss[0]), r, a, "1 %s J_s ds" % kind)


def test_born_superposition_and_null_source(hip_ops, prob):
    """1: v and ds together give born_ref(v) + js_ref(ds); device tensors and host memory give the same bits; with dStf = NULL the bits
    are sepfwi_born's and fwi_ops.born's; the Python keyword gives the C ABI's bits."""
    pb, vs, dss, ref, alt = prob
    hip_ops.release()
    fn = pb["para_fname"]
    got = born_src(pb, fn, v=vs[0], ds=dss[0])
    gathers_held(got, add(ref["jv"][0], ref["js"][0]), add(alt["jv"][0], alt["js"][0]), "1 J_m v + J_s ds")
    host = born_src(pb, fn, v=vs[0], ds=dss[0], host=True)
    assert all(np.array_equal(got[c], host[c]) for c in COMPS), "host memory"
    plain, null = born_src(pb, fn, v=vs[0], src_entry=False), born_src(pb, fn, v=vs[0], ds=None)
    assert all(np.array_equal(plain[c], null[c]) for c in COMPS), "dStf = NULL"
    assert any(not np.array_equal(plain[c], got[c]) for c in COMPS), "dStf changed nothing"
    m = [t.cuda() for t in pb["lame_init"]]
    py = hip_ops.born(*m, *cuda(vs[0]), pb["Stf"], 1, pb["Shot_ids"], fn, components=COMPS)
    assert all(np.array_equal(np.stack([d[c].cpu().numpy() for d in py]), plain[c]) for c in COMPS), "fwi_ops.born without dStf"
    py = hip_ops.born(*m, *cuda(vs[0]), pb["Stf"], 1, pb["Shot_ids"], fn, components=COMPS, dStf=torch.from_numpy(dss[0]))
    assert all(np.array_equal(np.stack([d[c].cpu().numpy() for d in py]), got[c]) for c in COMPS), "fwi_ops.born(dStf=)"
    py = hip_ops.born(*m, None, None, None, pb["Stf"], 1, pb["Shot_ids"], fn, components=COMPS, dStf=torch.from_numpy(dss[0]).cuda())
    alone = born_src(pb, fn, ds=dss[0])
    assert all(np.array_equal(np.stack([d[c].cpu().numpy() for d in py]), alone[c]) for c in COMPS), "fwi_ops.born(None, None, None, dStf=)"
    with pytest.raises(ValueError, match="all be given or all be None"):
        hip_ops.born(m[0], m[1], m[2], cuda(vs[0])[0], None, None, pb["Stf"], 1, pb["Shot_ids"], fn, dStf=torch.from_numpy(dss[0]))
    with pytest.raises(ValueError, match="shape of Stf"):
        hip_ops.born(*m, None, None, None, pb["Stf"], 1, pb["Shot_ids"], fn, dStf=torch.from_numpy(dss[0][:1]))


# ---- 2. the dot product, J outside the GPU -----------------------------------------------------------------------------------------------
def random_w(pb, seed, comps=("ett",)):
    rng = np.random.default_rng(seed)
    return {c: rng.uniform(-1.0, 1.0, (int(pb["Shot_ids"].numel()), pb["nrec"], pb["nSteps"])).astype(np.float32) for c in comps}


def test_dot_product_of_the_source_block(hip_ops, prob):
    """2: for random w, <js_ref(ds), w> = <ds, g_stf> per shot, and <born_ref(v) + js_ref(ds), w> = <v, g_m> + <ds, g_stf>; g_m has
    sepfwi_adjoint_exact's bits; device tensors and host memory give the same bits."""
    pb, vs, dss, ref, alt = prob
    hip_ops.release()
    fn = pb["para_fname"]
    w = random_w(pb, 11)
    g, gs, _ = exact_src(pb, fn, w=w)
    assert gs.shape == (2, pb["nSteps"]) and np.isfinite(gs).all() and not np.any(gs[:, -1]) and np.abs(gs).max() > 0
    g0, none, _ = exact_src(pb, fn, w=w, gstf=False, src_entry=False)
    assert all(np.array_equal(x, y) for x, y in zip(g, g0)), "g_m must keep sepfwi_adjoint_exact's bits"
    gh, gsh, _ = exact_src(pb, fn, w=w, host=True)
    assert all(np.array_equal(x, y) for x, y in zip(g, gh)) and np.array_equal(gs, gsh), "host memory"
    for k, ds in enumerate(dss):
        loc = S.local_rows(ds, pb["Shot_ids"].numpy())
        for i in range(2):
            r, a = X.data_dot(shot(ref["js"][k], i), shot(w, i)), X.data_dot(shot(alt["js"][k], i), shot(w, i))
            held(S.stf_dot(loc, gs, [i]), r, a, "2 <ds%d, g_stf> of shot %d" % (k, i), scale=norm(shot(ref["js"][k], i)) * norm(shot(w, i)))
        u, ua = add(ref["jv"][k], ref["js"][k]), add(alt["jv"][k], alt["js"][k])
        held(X.model_dot(vs[k], g) + S.stf_dot(loc, gs), X.data_dot(u, w), X.data_dot(ua, w), "2 joint <[v%d; ds%d], J^T w>" % (k, k),
             scale=norm(u) * norm(w))
    py = hip_ops.born_adjoint(*[t.cuda() for t in pb["lame_init"]], [{"ett": torch.from_numpy(w["ett"][i])} for i in range(2)], pb["Stf"], 1,
                              pb["Shot_ids"], fn, with_source=True)
    assert len(py) == 4 and all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(py[:3], g)) and np.array_equal(py[3].numpy(), gs)


@pytest.mark.parametrize("near", [False, True])
def test_unit_spikes_find_an_off_by_one(tmp_path, oracle, oracle_nvfma, hip_ops, prob, near):
    """2: ds a spike at it = 0, 1, nSteps-2, nSteps-1: amp g_stf[shot, it] = <js_ref(spike), w> per shot.  it = nSteps-1 never enters the
    forward pass: exactly 0 on both sides; so does it = 0, where the end taper is 0.  near: the fibre on the source's row, so that the
    spike at nSteps-2 reaches the channels within the record (on the default problem both sides of it are exact zeros)."""
    pb = P.make_problem(str(tmp_path), rec_z=2) if near else prob[0]
    hip_ops.release()
    fn, nS, stf = pb["para_fname"], pb["nSteps"], pb["Stf"].numpy()
    w = random_w(pb, 12)
    _, gs, _ = exact_src(pb, fn, w=w)
    amp = float(np.abs(stf).max())
    for it in (0, 1, nS - 2, nS - 1):
        sp = S.spike(stf, it)
        r, a = js(oracle, pb, sp), js(oracle_nvfma, pb, sp)
        for i in range(2):
            ref, alt, got = X.data_dot(shot(r, i), shot(w, i)), X.data_dot(shot(a, i), shot(w, i)), amp * float(gs[i, it])
            if it in (0, nS - 1):
                print("source adjoint 2 spike at %d, shot %d: got %r, reference %r" % (it, i, got, ref))
                assert got == 0.0 and ref == 0.0 and not np.any(r["ett"][i]), (it, i, got, ref)
                continue
            scale = norm(shot(r, i)) * norm(shot(w, i))
            if scale == 0.0:      # the spike does not reach the channels within the record: exact zeros on both sides
                assert not near and it == nS - 2 and got == 0.0 and ref == 0.0, (it, i, got, ref)
                continue
            held(got, ref, alt, "2 spike at %d%s, shot %d" % (it, " (fibre on the source's row)" if near else "", i), scale=scale)
    if near:      # the detector is live: the last-but-one spike is seen by the channels
        assert norm(js(oracle, pb, S.spike(stf, nS - 2))) > 0


# ---- 3. the product ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", WEIGHTS)
def test_product_with_the_source_block(hip_ops, prob, weights):
    """3: u^T H u = |W^1/2 J u|^2 for u = [v; ds], [0; ds], [v; 0]; <u1, H u2> = <H u1, u2> and both equal <W J u1, J u2>; the model
    blocks of [v; 0] are the existing product's bits."""
    pb, vs, dss, ref, alt = prob
    hip_ops.release()
    tag = "w%d" % WEIGHTS.index(weights)
    fn, _ = write_para(pb, "prod_" + tag, weights=None if weights == (1.0, 0.0, 0.0) else weights)
    ids = pb["Shot_ids"].numpy()
    loc = [S.local_rows(d, ids) for d in dss]
    n2 = lambda a: X.data_dot(a, a, weights)
    u, ua = [add(ref["jv"][k], ref["js"][k]) for k in (0, 1)], [add(alt["jv"][k], alt["js"][k]) for k in (0, 1)]
    H = [exact_src(pb, fn, v=vs[k], ds=dss[k])[:2] for k in (0, 1)]
    for k in (0, 1):
        hv, hs = H[k]
        X.outside_is_zero(pb, hv, "product")
        assert not np.any(hs[:, -1]) and np.isfinite(hs).all()
        held(X.model_dot(vs[k], hv) + S.stf_dot(loc[k], hs), n2(u[k]), n2(ua[k]), "3 %s u^T H u, u = [v%d; ds%d]" % (tag, k, k))
    hv, hs, _ = exact_src(pb, fn, v=None, ds=dss[0])
    held(S.stf_dot(loc[0], hs), n2(ref["js"][0]), n2(alt["js"][0]), "3 %s u^T H u, u = [0; ds0]" % tag)
    cr, ca = X.data_dot(ref["jv"][1], ref["js"][0], weights), X.data_dot(alt["jv"][1], alt["js"][0], weights)
    held(X.model_dot(vs[1], hv), cr, ca, "3 %s <[v1; 0], H [0; ds0]> against <W J_m v1, J_s ds0>" % tag, scale=float(np.sqrt(n2(ref["jv"][1]) * n2(ref["js"][0]))))
    hv, hs, _ = exact_src(pb, fn, v=vs[0], ds=None)
    held(X.model_dot(vs[0], hv), n2(ref["jv"][0]), n2(alt["jv"][0]), "3 %s u^T H u, u = [v0; 0]" % tag)
    old, _, _ = exact_src(pb, fn, v=vs[0], gstf=False, src_entry=False)
    assert all(np.array_equal(x, y) for x, y in zip(hv, old)), "[v; 0]: the model blocks must keep the existing product's bits"
    held(S.stf_dot(loc[1], hs), X.data_dot(ref["js"][1], ref["jv"][0], weights), X.data_dot(alt["js"][1], alt["jv"][0], weights),
         "3 %s <[0; ds1], H [v0; 0]> against <W J_s ds1, J_m v0>" % tag, scale=float(np.sqrt(n2(ref["js"][1]) * n2(ref["jv"][0]))))
    c12 = X.model_dot(vs[0], H[1][0]) + S.stf_dot(loc[0], H[1][1])
    c21 = X.model_dot(vs[1], H[0][0]) + S.stf_dot(loc[1], H[0][1])
    cr, ca = X.data_dot(u[0], u[1], weights), X.data_dot(ua[0], ua[1], weights)
    scale = float(np.sqrt(n2(u[0]) * n2(u[1])))
    held(c12, c21, c21 + (ca - cr), "3 %s symmetry <u1, H u2> against <H u1, u2>" % tag, scale=scale)
    held(c12, cr, ca, "3 %s <u1, H u2> against <W J u1, J u2>" % tag, scale=scale)


# ---- 4. the gradient mode ------------------------------------------------------------------------------------------------------------------
def test_gradient_of_the_misfit_with_respect_to_the_source(oracle, oracle_nvfma, hip_ops, prob):
    """4: observed data from lame_true (the oracle's), synthetics at lame_init: <gStf, ds> = -sum_c w_c <obs_c - syn_c, js_ref(ds)_c>,
    every term from the oracle; the misfit is exactly quadratic in stf: f(stf + p) = f(stf) + <gStf, p> + 1/2 <p, H_ss p> through the
    Python surface (1e-4 of f(stf)); the misfit, its parts and an armed pseudo-Hessian are untouched."""
    from sepfwi import _native
    pb, vs, dss, ref, alt = prob
    hip_ops.release()
    fn, _ = write_para(pb, "srcgrad")
    obs, r, mis = X.oracle_residuals(oracle, pb)
    _, r_alt, _ = X.oracle_residuals(oracle_nvfma, pb)
    for i, sid in enumerate(pb["Shot_ids"].tolist()):
        hip_ops.set_observed(fn, sid, torch.from_numpy(np.ascontiguousarray(obs["ett"][i])))
    m = [t.cuda() for t in pb["lame_init"]]
    Stf, ids = pb["Stf"], pb["Shot_ids"]
    before = hip_ops.backward(*m, Stf, 1, ids, fn, pseudo_hessian=2)
    parts = hip_ops.misfit_parts(fn)

    def read_ph():
        Hh = torch.empty((3,) + tuple(m[0].shape), dtype=torch.float32)
        _native.check(_native.lib().sepfwi_get_pseudo_hessian(fn.encode(), 0, *[C.c_void_p(Hh[k].data_ptr()) for k in range(3)]))
        return Hh

    ph = read_ph()
    out = hip_ops.backward(*m, Stf, 1, ids, fn, exact_adjoint=True, source_gradient=True)
    gS = out[4].numpy()
    assert len(out) == 5 and gS.shape == tuple(Stf.shape) and np.abs(gS).max() > 0 and not np.any(gS[:, -1])
    assert torch.equal(out[0].cpu(), before[0].cpu()) and abs(float(out[0]) - mis) <= 1e-4 * mis
    assert hip_ops.misfit_parts(fn) == parts and torch.equal(read_ph(), ph)
    plain = hip_ops.backward(*m, Stf, 1, ids, fn, exact_adjoint=True)
    assert not torch.any(plain[4]) and all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(plain[:4], out[:4])), "the model blocks keep their bits"
    neg = lambda q: {c: -np.asarray(q[c]) for c in COMPS}
    tests = [("ds0", dss[0], ref["js"][0], alt["js"][0]), ("ds1", dss[1], ref["js"][1], alt["js"][1])]
    wav = np.ascontiguousarray(0.02 * Stf.numpy())      # a change of the wavelet's amplitude: J_s of it is 0.02 syn, far from orthogonal to r
    tests.append(("0.02 stf", wav, js(oracle, pb, wav), js(oracle_nvfma, pb, wav)))
    for name, ds, jr, ja in tests:
        rr, aa = X.data_dot(jr, neg(r)), X.data_dot(ja, neg(r_alt))
        held(S.stf_dot(ds, gS), rr, aa, "4 <gStf, %s> (cosine %.3f)" % (name, rr / (norm(jr) * norm(r))), scale=abs(rr))
    # exactly quadratic in stf
    p = torch.from_numpy(S.draw_ds(5, Stf.numpy(), 0.2))
    f = lambda s: float(hip_ops.forward(*m, s, 0, ids, fn)[0])
    f0, f1 = f(Stf), f((Stf + p).contiguous())
    hp = hip_ops.gauss_newton(*m, None, None, None, Stf, 1, ids, fn, exact=True, dStf=p)
    assert len(hp) == 4 and hp[3].shape == Stf.shape
    lin, quad = S.stf_dot(gS, p.numpy()), 0.5 * S.stf_dot(hp[3].numpy(), p.numpy())
    print("source adjoint 4 quadratic: f(stf) %.8e, f(stf + p) %.8e, <gStf, p> %.8e, 1/2 <p, H p> %.8e, deviation %.2e of f(stf)"
          % (f0, f1, lin, quad, abs(f1 - (f0 + lin + quad)) / f0))
    assert abs(lin) > 1e-2 * f0 and quad > 1e-2 * f0, "the perturbation decides nothing"
    assert abs(f1 - (f0 + lin + quad)) <= FC.MISFIT_TOL * f0
    after = hip_ops.backward(*m, Stf, 1, ids, fn, pseudo_hessian=2)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(before, after))
    with pytest.raises(ValueError, match="exact=True"):
        hip_ops.gauss_newton(*m, *cuda(vs[0]), Stf, 1, ids, fn, dStf=p)
    with pytest.raises(ValueError, match="exact_adjoint=True"):
        hip_ops.backward(*m, Stf, 1, ids, fn, source_gradient=True)


# ---- 5. the surface ------------------------------------------------------------------------------------------------------------------------
def test_surface_layouts_and_launch_counts(oracle, hip_ops, prob):
    """5: gStf comes in Stf's shape with zero rows for shots not in Shot_ids, and is the C ABI's local row; a call with and without the
    source arguments issues the same launches."""
    pb, vs, dss, ref, alt = prob
    hip_ops.release()
    fn, _ = write_para(pb, "surface")
    obs, _, _ = X.oracle_residuals(oracle, pb)
    for i, sid in enumerate(pb["Shot_ids"].tolist()):
        hip_ops.set_observed(fn, sid, torch.from_numpy(np.ascontiguousarray(obs["ett"][i])))
    m = [t.cuda() for t in pb["lame_init"]]
    one = torch.tensor([1], dtype=torch.int32)
    out = hip_ops.backward(*m, pb["Stf"], 1, one, fn, exact_adjoint=True, source_gradient=True)
    n0 = hip_ops.stats(fn)["launches"]
    zero = hip_ops.backward(*m, pb["Stf"], 1, one, fn, exact_adjoint=True)
    n1 = hip_ops.stats(fn)["launches"]
    assert not torch.any(zero[4]) and zero[4].shape == pb["Stf"].shape
    gS = out[4].numpy()
    assert gS.shape == tuple(pb["Stf"].shape) and not np.any(gS[0]) and np.abs(gS[1]).max() > 0
    _, loc, _ = exact_src(pb, fn, ids=[1])
    assert loc.shape == (1, pb["nSteps"]) and np.array_equal(loc[0], gS[1]), "the local layout: row i belongs to shot_ids[i]"
    _, loch, _ = exact_src(pb, fn, ids=[1], host=True)
    assert np.array_equal(loc, loch), "host memory"
    print("source adjoint 5: launches of the gradient mode with / without g_stf: %d / %d" % (n0, n1))
    assert n0 == n1
    hv = hip_ops.gauss_newton(*m, *cuda(vs[0]), pb["Stf"], 1, one, fn, exact=True, dStf=torch.from_numpy(dss[0]))
    n2 = hip_ops.stats(fn)["launches"]
    hip_ops.gauss_newton(*m, *cuda(vs[0]), pb["Stf"], 1, one, fn, exact=True)
    n3 = hip_ops.stats(fn)["launches"]
    print("source adjoint 5: launches of the product with / without the source block: %d / %d" % (n2, n3))
    assert n2 == n3 and len(hv) == 4 and not torch.any(hv[3][0]) and torch.any(hv[3][1])
    st = hip_ops.stats(fn)
    assert st["bwd_steps"] == pb["nSteps"] - 1 and "exact adjoint" in hip_ops.loop_status(fn)


# ---- 7. the example ------------------------------------------------------------------------------------------------------------------------
def test_source_inversion_example_reduces_the_misfit(tmp_path):
    """7: examples/source_inversion.py at the small problem size: the misfit along the CG iterates never increases and ends below the
    initial one (the ratio is printed, not asserted)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "source_inversion.py"), "--device", "cuda", "--small", "--workdir", str(tmp_path)],
                         capture_output=True, text=True, timeout=300, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    lines = out.stdout.splitlines()
    f = [float(ln.split("misfit")[1].split()[0]) for ln in lines if ln.startswith("cg ") and "misfit" in ln]
    assert len(f) >= 3 and all(b <= a for a, b in zip(f, f[1:])), f
    assert f[-1] < f[0], f
    print("source inversion example: final / initial misfit = %.3e" % (f[-1] / f[0]))
    assert any(ln.startswith("done: ") for ln in lines)
