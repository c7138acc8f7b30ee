"""The exact discrete adjoint on the GPU (-m gpu): csrc/exact_adjoint.hip and csrc/session_exact.cpp through sepfwi_adjoint_exact and
fwi_ops.gauss_newton(exact=True) / born_adjoint / backward(exact_adjoint=True), against J itself outside the GPU
(tests/exact_adjoint_ref.py: <J_ref v, w> in float64, nothing on the adjoint side restated).

Tolerance, none new: the suite's gradient tolerance 1e-3, relative, plus 3 x the difference of the same reference quantity between the two
oracle builds (plain and nvfma), the yardstick of tests/fuzz_common.py for float32 rounding:
    |got - ref| <= 1e-3 |ref| + 3 |alt - ref|
Every dot product is accumulated in float64 on the host.  Each comparison prints its deviation before it asserts
(profiles/r11_exact_adjoint.txt holds the figures measured on the MI355X).  The problems here are hand-picked;
tests/test_gpu_exact_adjoint_fuzz.py holds the same identities on seeded random geometries (channels inside the absorbing layers, ragged
channel counts with the caller's w, w in host memory, joint and gauge misfits).

Every test fails on the parent (the entry point is missing); 1, 3, 4 and 6 would also fail on the parent's adjoint if it were merely
re-exported: v^T H v / |W^1/2 J v|^2 reads 0.9923 and 0.9844 there on the fixed problems, residual column nSteps-1 is dropped."""
import ctypes as C

import numpy as np
import pytest
import torch

import exact_adjoint_ref as X
import problems as P
import pseudo_hessian_ref as R
from exact_adjoint_ref import PROBE_CELLS, WEIGHTS, capi, cuda, held, outside_is_zero
from fuzz_common import write_para
from gauge_ref import gauge_of, member_survey

pytestmark = pytest.mark.gpu
TOL = X.TOL
COMPS = X.COMPS


def weight_keys(w):
    return {} if w == (1.0, 0.0, 0.0) else dict(misfit_w_ett=w[0], misfit_w_vx=w[1], misfit_w_vz=w[2])


def gn(hip_ops, pb, v, fn=None, exact=True, ids=None):
    hv = hip_ops.gauss_newton(*[t.cuda() for t in pb["lame_init"]], *cuda(v), pb["Stf"], 1, pb["Shot_ids"] if ids is None else ids,
                              fn or pb["para_fname"], exact=exact)
    return [h.cpu().numpy() for h in hv]


def gpu_jv(hip_ops, pb, v, fn=None):
    out = hip_ops.born(*[t.cuda() for t in pb["lame_init"]], *cuda(v), pb["Stf"], 1, pb["Shot_ids"], fn or pb["para_fname"], components=COMPS)
    return {c: np.stack([d[c].cpu().numpy() for d in out]) for c in COMPS}


def jtw(hip_ops, pb, w, fn=None, ids=None):
    """w: {component: (nshots, nrec, nSteps)} -> [gLambda, gMu, gDen] numpy"""
    ids = pb["Shot_ids"] if ids is None else ids
    per_shot = [{c: torch.from_numpy(np.ascontiguousarray(a[i], dtype=np.float32)) for c, a in w.items()} for i in range(int(ids.numel()))]
    g = hip_ops.born_adjoint(*[t.cuda() for t in pb["lame_init"]], per_shot, pb["Stf"], 1, ids, fn or pb["para_fname"])
    return [a.cpu().numpy() for a in g]


@pytest.fixture(scope="module")
def prob_a(oracle, oracle_nvfma, hip_ops, tmp_path_factory):
    """PROBLEM_A: 50 x 90 (two row segments per row, the last ragged; both layers), two shots.  The three v of test 1 on Omega and J_ref v
    of each on both oracle builds, computed once and left unchanged."""
    pb = P.make_problem(str(tmp_path_factory.mktemp("exact_a")), **R.PROBLEM_A)
    vs = [X.smooth_v(pb, 3), X.smooth_v(pb, 4), X.white_v(pb, 5)]
    ref = [X.jv_ref(oracle, pb, v) for v in vs]
    alt = [X.jv_ref(oracle_nvfma, pb, v) for v in vs]
    return pb, vs, ref, alt


@pytest.mark.parametrize("weights", WEIGHTS)
def test_gauss_newton_product_is_symmetric_and_equals_the_norm_of_jv(hip_ops, prob_a, weights):
    """1: v^T H v = |W^1/2 J_ref v|^2 for two smooth v and white noise on Omega; <v2, H v1> = <v1, H v2>; the same v^T H v against the
    GPU's own Born gathers; hv exactly 0 outside Omega; exact=False is the parent's product, bit for bit."""
    pb, vs, ref, alt = prob_a
    hip_ops.release()
    tag = "w%d" % WEIGHTS.index(weights)
    fn, _ = write_para(pb, "gn_" + tag, **weight_keys(weights))
    hv = [gn(hip_ops, pb, v, fn) for v in vs]
    vhv = [X.model_dot(v, h) for v, h in zip(vs, hv)]
    for k, name in enumerate(("smooth 3", "smooth 4", "white noise")):
        outside_is_zero(pb, hv[k], name)
        held(vhv[k], X.data_dot(ref[k], ref[k], weights), X.data_dot(alt[k], alt[k], weights), "1 %s v^T H v, %s" % (tag, name))
        own = gpu_jv(hip_ops, pb, vs[k], fn)
        n_own = X.data_dot(own, own, weights)
        held(vhv[k], n_own, n_own, "1 %s v^T H v against the GPU's own J v, %s" % (tag, name))
    scale = float(np.sqrt(vhv[0] * vhv[1]))
    c21, c12 = X.model_dot(vs[1], hv[0]), X.model_dot(vs[0], hv[1])
    cr, ca = X.data_dot(ref[0], ref[1], weights), X.data_dot(alt[0], alt[1], weights)
    held(c21, c12, c12 + (ca - cr), "1 %s symmetry <v2, H v1> against <v1, H v2>" % tag, scale=scale)
    held(c21, cr, ca, "1 %s <v2, H v1> against <W J v1, J v2>" % tag, scale=scale)
    old = gn(hip_ops, pb, vs[0], fn, exact=False)
    m = [t.cuda() for t in pb["lame_init"]]
    parent = hip_ops._born(*m, *cuda(vs[0]), pb["Stf"], 1, pb["Shot_ids"], fn, (), True)[1].cpu().numpy()
    assert all(np.array_equal(a, b) for a, b in zip(old, parent))
    assert any(not np.array_equal(a, b) for a, b in zip(old, hv[0])), "exact=True changed nothing"
    ratio = X.model_dot(vs[0], old) / X.data_dot(ref[0], ref[0], weights)
    print("exact adjoint 1 %s: the reference's adjoint on the same v: v^T H v / |W^1/2 J v|^2 = %.4f (exact: %.6f)"
          % (tag, ratio, vhv[0] / X.data_dot(ref[0], ref[0], weights)))


@pytest.mark.parametrize("param", [0, 1, 2])
def test_jtw_cell_by_cell(oracle, oracle_nvfma, hip_ops, prob_a, param):
    """2: w = J_ref v2 of one shot, (J^T w)_k against <J_ref e_k, w> at 8 cells of one parameter: 1e-3 relative L2 of the vector, and every
    entry within 1e-3 of the largest plus the yardstick."""
    pb, vs, ref, alt = prob_a
    g = []
    for sid in (0, 1):
        g.append(jtw(hip_ops, pb, {"ett": ref[1]["ett"][sid:sid + 1]}, ids=torch.tensor([sid], dtype=torch.int32)))
        outside_is_zero(pb, g[-1], "J^T w")
    scale = 0.01 * float(np.abs(pb["lame_init"][param].numpy()).mean())
    r = X.probe_dots(oracle, pb, param, PROBE_CELLS, ref[1], scale=scale)
    a = X.probe_dots(oracle_nvfma, pb, param, PROBE_CELLS, ref[1], scale=scale)
    got = np.array([float(g[sid][param][z, x]) for sid, z, x in PROBE_CELLS], np.float64)
    l2 = lambda q: float(np.linalg.norm(q))
    print("exact adjoint 2 parameter %d: rel-L2 of the 8 entries %.2e (the two oracle builds %.2e); entries got / ref:" % (param, l2(got - r) / l2(r), l2(a - r) / l2(r)))
    for c, x, y, y2 in zip(PROBE_CELLS, got, r, a):
        print("    cell %r: %.6e / %.6e, deviation %.2e of the largest (builds %.2e)" % (c, x, y, abs(x - y) / np.abs(r).max(), abs(y2 - y) / np.abs(r).max()))
    assert l2(r) > 0 and l2(got - r) <= TOL * l2(r) + 3.0 * l2(a - r)
    assert np.all(np.abs(got - r) <= TOL * np.abs(r).max() + 3.0 * np.abs(a - r))


def test_time_alignment(hip_ops, prob_a):
    """3: w = J_ref v2 in column nSteps-1 alone (the column the reference's pass drops): <v2, J^T w> is the reference's and not 0; in
    column 0 alone: J^T w is exactly 0; in column 1 alone."""
    pb, vs, ref, alt = prob_a
    nS = pb["nSteps"]

    def column(src, k):
        w = np.zeros_like(src["ett"])
        w[:, :, k] = src["ett"][:, :, k]
        return {"ett": w}

    w = column(ref[1], nS - 1)
    r, a = X.data_dot(ref[1], w), X.data_dot(alt[1], column(alt[1], nS - 1))
    assert r > 0
    held(X.model_dot(vs[1], jtw(hip_ops, pb, w)), r, a, "3 column nSteps-1")
    w0 = {"ett": np.zeros_like(ref[1]["ett"])}
    w0["ett"][:, :, 0] = np.random.default_rng(1).uniform(-1.0, 1.0, w0["ett"].shape[:2])
    assert all(not np.any(g) for g in jtw(hip_ops, pb, w0)), "column 0 must never be injected"
    mid = nS // 2     # (column 1 itself holds exact zeros on this problem: the wave has not left the source; tested, and a live column too)
    for k in (1, mid):
        w = column(ref[1], k)
        r, a = X.data_dot(ref[1], w), X.data_dot(alt[1], column(alt[1], k))
        held(X.model_dot(vs[1], jtw(hip_ops, pb, w)), r, a, "3 column %d" % k, scale=max(abs(r), 1e-300))


def test_exact_gradient_of_the_misfit(oracle, oracle_nvfma, hip_ops, prob_a):
    """4: observed data from lame_true (the oracle's gathers, installed with set_observed): <g, v> = <J_ref v, -r_oracle> for the three
    v; misfit = backward's, bit for bit; a following backward returns the bits it returned before; misfit parts and an armed
    pseudo-Hessian are untouched."""
    from sepfwi import _native
    pb, vs, ref, alt = prob_a
    hip_ops.release()
    fn, _ = write_para(pb, "grad")
    obs, r, mis = X.oracle_residuals(oracle, pb)
    _, r_alt, _ = X.oracle_residuals(oracle_nvfma, pb)
    for i, sid in enumerate(pb["Shot_ids"].tolist()):
        hip_ops.set_observed(fn, sid, torch.from_numpy(np.ascontiguousarray(obs["ett"][i])))
    m = [t.cuda() for t in pb["lame_init"]]
    before = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], fn, pseudo_hessian=2)
    parts = hip_ops.misfit_parts(fn)

    def read_ph():
        H = torch.empty((3,) + tuple(m[0].shape), dtype=torch.float32)
        _native.check(_native.lib().sepfwi_get_pseudo_hessian(fn.encode(), 0, *[C.c_void_p(H[k].data_ptr()) for k in range(3)]))
        return H

    ph = read_ph()
    out = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], fn, exact_adjoint=True)
    assert len(out) == 5 and not torch.any(out[4]) and out[4].shape == pb["Stf"].shape
    assert torch.equal(out[0].cpu(), before[0].cpu()), (float(out[0]), float(before[0]))
    assert abs(float(out[0]) - mis) <= 1e-4 * mis
    assert hip_ops.misfit_parts(fn) == parts and torch.equal(read_ph(), ph)
    assert "exact adjoint" in hip_ops.loop_status(fn)
    g = [t.cpu().numpy() for t in out[1:4]]
    outside_is_zero(pb, g, "exact gradient")
    neg = lambda q: {c: -np.asarray(q[c]) for c in COMPS}
    for k, name in enumerate(("smooth 3", "smooth 4", "white noise")):
        rr, aa = X.data_dot(ref[k], neg(r)), X.data_dot(alt[k], neg(r_alt))
        scale = float(np.sqrt(X.data_dot(ref[k], ref[k]) * X.data_dot(r, r)))      # |J v| |r|: the dot product of two unrelated gathers cancels
        held(X.model_dot(vs[k], g), rr, aa, "4 <g, v>, %s (cosine %.3f)" % (name, rr / scale), scale=abs(rr))
    after = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], fn, pseudo_hessian=2)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(before, after))


GEOMETRIES = {"strided": (dict(nrec_stride=3), {}, (1.0, 0.0, 0.0)), "vertical": (dict(das_fiber="vertical"), {}, (1.0, 0.0, 0.0)),
              "directional": (dict(das_sensitivity="random", nrec_stride=2), {}, (1.0, 0.0, 0.0)), "gauge3": (dict(nrec_stride=2), {}, (1.0, 0.0, 0.0)),
              "geophones": ({}, {}, (0.0, 1.0, 0.5))}


@pytest.mark.parametrize("kind", sorted(GEOMETRIES))
def test_receiver_geometries(tmp_path, oracle, oracle_nvfma, hip_ops, kind):
    """5: channels that are not a line, a vertical fibre, directional channels, gauge length 3 (reference: the member survey), vx / vz
    geophones without the strain -- the dot test of 1 with one smooth v."""
    kw, keys, weights = GEOMETRIES[kind]
    pb = P.make_problem(str(tmp_path), **dict(R.PROBLEM_A, **kw))
    keys = dict(keys, **weight_keys(weights))
    G = 3 if kind == "gauge3" else 0
    if G:
        keys["das_gauge_length"] = G * pb["para"]["dx"]
    fn, _ = write_para(pb, kind, **keys)
    v = X.smooth_v(pb, 11)

    def ref_side(lib):
        if not G:
            return X.jv_ref(lib, pb, v)
        mem = X.jv_ref(lib, pb, v, survey=member_survey(pb["survey"], G, False))
        return {"ett": gauge_of(mem["ett"], G), "vx": mem["vx"], "vz": mem["vz"]}      # (weights (1, 0, 0): the strain alone is used)

    r, a = ref_side(oracle), ref_side(oracle_nvfma)
    hip_ops.release()
    hv = gn(hip_ops, pb, v, fn)
    outside_is_zero(pb, hv, kind)
    held(X.model_dot(v, hv), X.data_dot(r, r, weights), X.data_dot(a, a, weights), "5 %s v^T H v" % kind)


LAYERS = {"square": {}, "dz_ne_dx": dict(dz=12.5), "npad0": dict(nPad=0), "npad5": dict(nPad=5), "water": {}}


@pytest.mark.parametrize("kind", sorted(LAYERS))
def test_absorbing_layers(tmp_path, oracle, oracle_nvfma, hip_ops, kind):
    """6: 40 x 48, nPml 10, 400 steps, source and fibre 4 cells from the layers -- most of the energy crosses them, which is where 1/K
    and a outside the stencil would show.  dz != dx, nPad 0 and 5, 12 rows of water on top (dMu = 0 there)."""
    pb = P.make_problem(str(tmp_path), nz=40, nx=48, nPml=10, nSteps=400, nshots=1, src_z=4, rec_z=35, src_x=[4], **LAYERS[kind])
    water = 0
    if kind == "water":
        water = pb["nPml"] + 12
        for key in ("lame_true", "lame_init"):
            lam, mu, den = pb[key]
            lam[:water, :] = 1000.0 * 1500.0 ** 2 / 1e6
            mu[:water, :] = 0.0
            den[:water, :] = 1000.0
    vs = [X.smooth_v(pb, 21, water), X.white_v(pb, 22, water)]
    ref, alt = [X.jv_ref(oracle, pb, v) for v in vs], [X.jv_ref(oracle_nvfma, pb, v) for v in vs]
    hip_ops.release()
    for v, r, a, name in zip(vs, ref, alt, ("smooth", "white noise")):
        hv = gn(hip_ops, pb, v)
        outside_is_zero(pb, hv[:1] + hv[2:], kind)      # (dMu is 0 in the water: hvMu need not be live on all of Omega)
        held(X.model_dot(v, hv), X.data_dot(r, r), X.data_dot(a, a), "6 %s v^T H v, %s" % (kind, name))
    scale = float(np.sqrt(X.data_dot(ref[0], ref[0]) * X.data_dot(ref[1], ref[1])))
    got = X.model_dot(vs[0], jtw(hip_ops, pb, {"ett": ref[1]["ett"]}))
    held(got, X.data_dot(ref[0], ref[1]), X.data_dot(alt[0], alt[1]), "6 %s <v1, J^T J_ref v2>" % kind, scale=scale)


def test_kernel_structures(probes_lib, hip_ops, prob_a):
    """7: bz, xcd_remap, rk_lazy change which thread updates which cell: the product keeps its bits; rho_fly and amu_fly change where an
    average comes from: the dot test stays within tolerance under each."""
    pb, vs, ref, alt = prob_a
    fn, _ = write_para(pb, "structures")
    r, a = X.data_dot(ref[0], ref[0]), X.data_dot(alt[0], alt[0])
    with P.kernel_options():
        base = gn(hip_ops, pb, vs[0], fn)
    held(X.model_dot(vs[0], base), r, a, "7 default structure")
    for opts in (dict(bz=1), dict(bz=4), dict(bz=8), dict(xcd_remap=0), dict(rk_lazy=0), dict(rho_fly=0), dict(amu_fly=0)):
        with P.kernel_options(**opts):
            assert all(probes_lib.sepfwi_get_option(k.encode()) == val for k, val in opts.items()), (opts, "the option is not in force")
            hv = gn(hip_ops, pb, vs[0], fn)
        held(X.model_dot(vs[0], hv), r, a, "7 %r" % (opts,))
        if "rho_fly" not in opts and "amu_fly" not in opts:
            assert all(np.array_equal(x, y) for x, y in zip(hv, base)), opts


def test_a_grid_of_loop_size(tmp_path, hip_ops):
    """8: 300 x 500, 420 steps, one shot (where a gradient call runs the persistent loop): v^T H v against the GPU's own J v -- the CPU
    reference is too slow here, so the yardstick is not available and the bound is 1e-3 alone.  Device tensors and host arrays through
    the C ABI give the same bits."""
    hip_ops.release()
    pb = P.make_problem(str(tmp_path), nz=300, nx=500, nPml=10, nSteps=420, nshots=1, hetero=True, rec_z=40)
    v = X.smooth_v(pb, 17)
    hv = gn(hip_ops, pb, v)
    st = hip_ops.stats(pb["para_fname"])
    assert st["bwd_steps"] == pb["nSteps"] - 1 and st["persist_steps"] == 0 and "exact adjoint" in hip_ops.loop_status(pb["para_fname"])
    outside_is_zero(pb, hv, "300 x 500")
    own = gpu_jv(hip_ops, pb, v)
    n_own = X.data_dot(own, own)
    held(X.model_dot(v, hv), n_own, n_own, "8 300 x 500 v^T H v against the GPU's own J v")
    model = [t.numpy() for t in pb["lame_init"]]
    rc, host = capi(pb, pb["para_fname"], model, v=v, host_out=True)
    assert rc == 0 and all(np.array_equal(x, y) for x, y in zip(host, hv))
    rc, dev = capi(pb, pb["para_fname"], [t.cuda() for t in pb["lame_init"]], v=cuda(v))
    assert rc == 0 and all(np.array_equal(x, y) for x, y in zip(dev, hv))
    print("exact adjoint 8: bwd_ms %.2f for %d steps (%.1f us per step), launches %d" % (st["bwd_ms"], st["bwd_steps"], 1e3 * st["bwd_ms"] / max(st["bwd_steps"], 1), st["launches"]))
    hip_ops.release()


def test_refusals_are_error_codes(tmp_path, hip_ops):
    """9: NULL outputs, a partial v, v and w together, a bad shot list, a w component without a weight, a live conditioning key -- each
    SEPFWI_EINVAL, none a fault; the session still works afterwards."""
    from sepfwi import _native
    L = _native.lib()
    pb = P.make_problem(str(tmp_path), nz=40, nx=48, nPml=10, nSteps=120, nshots=1)
    fn = pb["para_fname"]
    m = [t.cuda() for t in pb["lame_init"]]
    v = cuda(X.smooth_v(pb, 3))
    w = torch.zeros(pb["nrec"] * pb["nSteps"], dtype=torch.float32, device="cuda")
    g = [torch.zeros_like(m[0]) for _ in range(3)]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stf = pb["Stf"].contiguous()
    ids = np.zeros(1, np.int32)

    def call(g=g, w=(None, None, None), v=(None, None, None), model=m, n=1, idp=ids, fname=fn):
        return L.sepfwi_adjoint_exact(None, *[p(t) for t in g], *[p(t) for t in w], *[p(t) for t in v], *[p(t) for t in model], p(stf), 0, n,
                                      None if idp is None else C.c_void_p(idp.ctypes.data), fname.encode(), None)

    assert call(g=[g[0], None, g[2]]) == -1 and b"g_" in L.sepfwi_last_error()
    assert call(v=[v[0], None, v[2]]) == -1 and b"all NULL or all set" in L.sepfwi_last_error()
    assert call(v=v, w=[w, None, None]) == -1 and b"not both" in L.sepfwi_last_error()
    assert call(model=[m[0], None, m[2]]) == -1
    assert call(idp=None) == -1 and b"shot list" in L.sepfwi_last_error()
    assert call(idp=np.array([7], np.int32), w=[w, None, None]) == -1 and b"not in the survey" in L.sepfwi_last_error()
    assert call(w=[None, w, None]) == -1 and b"misfit_w_vx" in L.sepfwi_last_error()
    fc, _ = write_para(pb, "cond", if_cross_misfit=True)
    assert call(fname=fc, w=[w, None, None]) == -1 and b"conditioned" in L.sepfwi_last_error()
    with pytest.raises(_native.SepFwiError):
        hip_ops.gauss_newton(*m, *v, pb["Stf"], 1, pb["Shot_ids"], fc, exact=True)
    with pytest.raises(ValueError, match="ONE GPU"):
        hip_ops.gauss_newton(*m, *v, pb["Stf"], 2, pb["Shot_ids"], fn, exact=True)
    with pytest.raises(ValueError, match="one shape"):
        hip_ops.gauss_newton(*m, v[0][:-1], v[1], v[2], pb["Stf"], 1, pb["Shot_ids"], fn, exact=True)
    hv = hip_ops.gauss_newton(*m, *v, pb["Stf"], 1, pb["Shot_ids"], fn, exact=True)      # the session still works
    assert all(torch.isfinite(h).all() and h.abs().max() > 0 for h in hv)
