"""Gauss-Newton and the exact adjoint under windowed and band-passed data on the GPU (-m gpu): sepfwi_condition, and sepfwi_born /
sepfwi_adjoint_exact under a parameter file whose live conditioning keys are among if_win and filter, through fwi_ops.condition,
gauss_newton, born_adjoint and backward(exact_adjoint=True).  The yardstick is outside the GPU (tests/cond_gn_ref.py): J from
tests/born_ref.py, C and Z from the oracle's cond_window / cond_bandpass; nothing adjoint is restated
(tests/test_conditioned_gn_reference.py licenses it on the CPU).

Tolerances, none new:
  1        the suite's seismogram tolerance, 1e-4 of the gather's maximum, plus 3 x |oracle - oracle_nvfma| element by element; the
           dot test <C a, b> = <a, C^T b> on the GPU to 1e-4 of |C a| |b|
  2, 3, 7  tests/test_gpu_exact_adjoint.py's: |got - ref| <= 1e-3 scale + 3 |alt - ref| (exact_adjoint_ref.held; alt: the nvfma build);
           the misfit to the suite's 1e-4
  4        tests/test_gpu_born.py's: 10 x the float32 rounding of obs = syn - J v, 1e-7 max|syn| / max|J v|, of each array's maximum
Every comparison prints its deviation before it asserts; profiles/r18_conditioned_gauss_newton.txt holds the figures measured on the
MI355X, and what three deliberately wrong variants of the pass do to them.

Tests 2-4 run the three linear modes and, beyond them, a narrow low band alone (cond_gn_ref.narrow): the file on which a forgotten Z shows.

On the parent commit tests 2, 3, 4, 5 and 7 fail on the refusal of every conditioning key and test 1 for lack of the entry point."""
import contextlib
import ctypes as C
import importlib.util
import io
import os
import re

import numpy as np
import pytest
import torch

import cond_gn_ref as G
import exact_adjoint_ref as X
import stf_ref as S
from exact_adjoint_ref import cuda, held
from sepfwi import utils as ft

pytestmark = pytest.mark.gpu
GATHER_TOL, MISFIT_TOL = 1e-4, 1e-4
V_SEEDS = (3, 4)


def model(pb, which="lame_init"):
    return [t.cuda() for t in pb[which]]


def gn(hip_ops, pb, v, exact=True, dStf=None):
    out = hip_ops.gauss_newton(*model(pb), *(cuda(v) if v is not None else (None, None, None)), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact=exact,
                               dStf=None if dStf is None else torch.from_numpy(dStf))
    return [h.cpu().numpy() for h in out]


def flat(gathers):
    return torch.from_numpy(np.concatenate([np.asarray(g, np.float32).reshape(-1) for g in gathers]))


def unflat(t, like):
    a, out, off = t.cpu().numpy(), [], 0
    for g in like:
        out.append(a[off:off + g.size].reshape(g.shape))
        off += g.size
    return out


class Side:
    """the reference quantities of one problem on both oracle builds: J v per v (and per source perturbation), Z C J v"""

    def __init__(self, oracle, oracle_nvfma, pb, seeds=V_SEEDS, with_source=False):
        self.pb, self.libs = pb, (oracle, oracle_nvfma)
        self.vs = [X.smooth_v(pb, s) for s in seeds]
        stf = pb["Stf"].numpy()
        self.ds = [S.draw_ds(k, stf, S.DS_SCALE) for k in range(len(seeds))] if with_source else [None] * len(seeds)
        self.jv = [[G.jv_ett(lib, pb, v, ds) for v, ds in zip(self.vs, self.ds)] for lib in self.libs]       # [build][v][shot]
        self.cjv = [[G.inputs_discriminate(oracle, pb, jv, "%s, v %d" % (os.path.basename(pb["para_fname"]), k)) if b == 0 else G.C_all(lib, pb, jv)
                     for k, jv in enumerate(self.jv[b])] for b, lib in enumerate(self.libs)]
        self.zcjv = [[[G.Z(c) for c in cj] for cj in side] for side in self.cjv]

    def norm2(self, k, b=0):
        return G.dot(self.zcjv[b][k], self.zcjv[b][k])

    def cross(self, j, k, b=0):
        return G.dot(self.zcjv[b][j], self.zcjv[b][k])


@pytest.fixture(scope="module")
def sides(oracle, oracle_nvfma, hip_ops, tmp_path_factory):
    """the small problem under the three linear modes and the narrow band, the two v of tests 2-4 and their reference sides: computed once, left unchanged"""
    out = {}
    for mode in G.ALL_MODES:
        pb = G.linear_problem(tmp_path_factory.mktemp("cgn_" + mode), mode)
        out[mode] = Side(oracle, oracle_nvfma, pb)
    return out


# ---- 1: sepfwi_condition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.MODES)
def test_condition_is_the_oracle_s_c(oracle, oracle_nvfma, hip_ops, sides, mode):
    """1: C of the file on the reference's J v against the oracle's, device and host pointers bit for bit, the per-shot dict form, and the
    dot test of C against C^T on the GPU with white noise."""
    s = sides[mode]
    pb, d = s.pb, s.jv[0][0]
    ref, alt = s.cjv[0][0], s.cjv[1][0]
    dev = hip_ops.condition(flat(d).cuda(), pb["Shot_ids"], pb["para_fname"])
    host = hip_ops.condition(flat(d), pb["Shot_ids"], pb["para_fname"])
    assert dev.is_cuda and not host.is_cuda and torch.equal(dev.cpu(), host), "host and device pointers differ"
    got = unflat(host, d)
    for i, (g, r, a) in enumerate(zip(got, ref, alt)):
        top = float(np.abs(r).max())
        worst = float(np.abs(g - r).max()) / top
        print("conditioned GN 1 %s shot %d: C d against the oracle's, max-norm deviation %.2e of the maximum (the two oracle builds %.2e)"
              % (mode, i, worst, float(np.abs(a - r).max()) / top))
        assert top > 0 and np.all(np.abs(g.astype(np.float64) - r) <= GATHER_TOL * top + 3.0 * np.abs(a.astype(np.float64) - r)), (mode, i, worst)
    per_shot = [{"ett": torch.from_numpy(np.ascontiguousarray(g)).cuda()} for g in d]
    as_dicts = hip_ops.condition(per_shot, pb["Shot_ids"], pb["para_fname"])
    assert all(np.array_equal(x["ett"].cpu().numpy(), y) for x, y in zip(as_dicts, got)) and all(torch.equal(p["ett"].cpu(), torch.from_numpy(g)) for p, g in zip(per_shot, d))
    rng = np.random.default_rng(21)
    a, b = [[rng.standard_normal(g.shape).astype(np.float32) for g in d] for _ in range(2)]
    ca = unflat(hip_ops.condition(flat(a).cuda(), pb["Shot_ids"], pb["para_fname"]), d)
    ctb = unflat(hip_ops.condition(flat(b).cuda(), pb["Shot_ids"], pb["para_fname"], transpose=True), d)
    lhs, rhs, scale = G.dot(ca, b), G.dot(a, ctb), G.norm(ca) * G.norm(b)
    print("conditioned GN 1 %s: <C a, b> %.8e, <a, C^T b> %.8e on the GPU, gap %.2e of |C a| |b|" % (mode, lhs, rhs, abs(lhs - rhs) / scale))
    assert scale > 0 and abs(lhs - rhs) <= GATHER_TOL * scale
    cb = unflat(hip_ops.condition(flat(b).cuda(), pb["Shot_ids"], pb["para_fname"]), d)
    if mode == "both":      # (window and filter do not commute: with C in the place of C^T the dot test above fails)
        assert abs(lhs - G.dot(a, cb)) > GATHER_TOL * scale


def test_condition_without_keys_is_the_identity(hip_ops, sides):
    """1: a file without conditioning keys: bit for bit the input, C and C^T, host and device; a wrong size is a ValueError."""
    s = sides["both"]
    pb = G.set_mode(s.pb, "none")
    d = flat(s.jv[0][0])
    for t in (d, d.cuda()):
        for tr in (False, True):
            out = hip_ops.condition(t, pb["Shot_ids"], pb["para_fname"], transpose=tr)
            assert out.data_ptr() != t.data_ptr() and torch.equal(out.cpu(), d)
    with pytest.raises(ValueError, match="elements"):
        hip_ops.condition(d[:-1], pb["Shot_ids"], pb["para_fname"])


# ---- 2: the exact product -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.ALL_MODES)
def test_exact_product_is_symmetric_and_equals_the_norm_of_zcjv(hip_ops, sides, mode):
    """2: v^T g = |Z C J v|^2 for two smooth v on Omega; <v2, H v1> = <v1, H v2>, and both = <Z C J v1, Z C J v2>."""
    s = sides[mode]
    pb = s.pb
    hip_ops.release()
    hv = [gn(hip_ops, pb, v) for v in s.vs]
    vhv = [X.model_dot(v, h) for v, h in zip(s.vs, hv)]
    for k in range(2):
        X.outside_is_zero(pb, hv[k], mode)
        held(vhv[k], s.norm2(k), s.norm2(k, 1), "conditioned GN 2 %s v^T H v, v %d" % (mode, k))
    scale = float(np.sqrt(vhv[0] * vhv[1]))
    c21, c12 = X.model_dot(s.vs[1], hv[0]), X.model_dot(s.vs[0], hv[1])
    cr, ca = s.cross(0, 1), s.cross(0, 1, 1)
    held(c21, c12, c12 + (ca - cr), "conditioned GN 2 %s symmetry <v2, H v1> against <v1, H v2>" % mode, scale=scale)
    held(c21, cr, ca, "conditioned GN 2 %s <v2, H v1> against <Z C J v1, Z C J v2>" % mode, scale=scale)


@pytest.mark.parametrize("mode", ["filter", "window"])
def test_exact_product_with_the_source_block(oracle, oracle_nvfma, hip_ops, sides, mode):
    """2: u = [P v; ds]: u^T H u = |Z C (J_m v + J_s ds)|^2 and the symmetry, the source block included.  (Under window AND filter the
    gain of the one and the loss of the other cancel on J_s ds, |C J u| = 0.97 |J u|: that file does not meet the conditions on the
    inputs for this u, so the two keys are taken one at a time.)"""
    pb = sides[mode].pb
    s = Side(oracle, oracle_nvfma, pb, with_source=True)
    hip_ops.release()
    out = [gn(hip_ops, pb, v, dStf=ds) for v, ds in zip(s.vs, s.ds)]
    assert all(len(o) == 4 and np.abs(o[3]).max() > 0 for o in out)
    udot = lambda k, o: X.model_dot(s.vs[k], o[:3]) + S.stf_dot(s.ds[k], o[3])
    uhu = [udot(k, out[k]) for k in range(2)]
    for k in range(2):
        held(uhu[k], s.norm2(k), s.norm2(k, 1), "conditioned GN 2 %s, [v; ds] u^T H u, u %d" % (mode, k))
    scale = float(np.sqrt(uhu[0] * uhu[1]))
    c21, c12 = udot(1, out[0]), udot(0, out[1])
    cr, ca = s.cross(0, 1), s.cross(0, 1, 1)
    held(c21, c12, c12 + (ca - cr), "conditioned GN 2 %s, [v; ds] symmetry" % mode, scale=scale)
    held(c21, cr, ca, "conditioned GN 2 %s, [v; ds] <u2, H u1> against the reference" % mode, scale=scale)


# ---- 3: the exact gradient ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.ALL_MODES)
def test_exact_gradient_of_the_conditioned_misfit(oracle, oracle_nvfma, hip_ops, sides, mode):
    """3: observed data from lame_true (the oracle's raw gathers, installed with set_observed; the session conditions them):
    <g, v> = -<Z C J v, Z (C obs - C syn)>; the misfit is a misfit call's on the same file; <g_stf, ds> against J_s ds in the same way."""
    s = sides[mode]
    pb = s.pb
    hip_ops.release()
    res, mis = [], []
    for lib in s.libs:
        obs, _ = G.oracle_gathers(lib, pb, "lame_true")
        syn, _ = G.oracle_gathers(lib, pb, "lame_init")
        r, m_ = G.conditioned_residual(lib, pb, obs, syn)
        res.append(r)
        mis.append(m_)
        if lib is s.libs[0]:
            for i, sid in enumerate(G.shots_of(pb)):
                hip_ops.set_observed(pb["para_fname"], sid, torch.from_numpy(np.ascontiguousarray(obs[i])))
    m = model(pb)
    f0 = float(hip_ops.forward(*m, pb["Stf"], 0, pb["Shot_ids"], pb["para_fname"])[0])
    out = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact_adjoint=True, source_gradient=True)
    f = float(out[0])
    print("conditioned GN 3 %s: misfit of the exact pass %.8e, of a misfit call %.8e (relative gap %.2e), of the oracle %.8e (%.2e)"
          % (mode, f, f0, abs(f - f0) / f0, mis[0], abs(f - mis[0]) / mis[0]))
    assert abs(f - f0) <= MISFIT_TOL * f0 and abs(f - mis[0]) <= MISFIT_TOL * mis[0] + 3.0 * abs(mis[1] - mis[0])
    g = [t.cpu().numpy() for t in out[1:4]]
    X.outside_is_zero(pb, g, "exact gradient " + mode)
    for k in range(2):
        rr, aa = -G.dot(s.zcjv[0][k], res[0]), -G.dot(s.zcjv[1][k], res[1])
        cosine = rr / np.sqrt(s.norm2(k) * G.dot(res[0], res[0]))
        held(X.model_dot(s.vs[k], g), rr, aa, "conditioned GN 3 %s <g, v>, v %d (cosine %.3f)" % (mode, k, cosine), scale=abs(rr))
    gs = out[4].numpy()
    assert gs.shape == tuple(pb["Stf"].shape) and np.abs(gs).max() > 0
    ds = S.draw_ds(0, pb["Stf"].numpy(), S.DS_SCALE)
    side = []
    for lib, r in zip(s.libs, res):
        zc = [G.Z(c) for c in G.C_all(lib, pb, G.jv_ett(lib, pb, None, ds))]
        side.append(-G.dot(zc, r))
    held(S.stf_dot(ds, gs), side[0], side[1], "conditioned GN 3 %s <g_stf, ds>" % mode, scale=abs(side[0]))


# ---- 4: the reference-style product ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.ALL_MODES)
def test_reference_style_product_is_the_gradient_at_shifted_data(hip_ops, sides, mode):
    """4: gauss_newton(exact=False) under the file against backward of a SECOND session of the same keys whose observed data are
    syn - J v (both from the GPU, raw).  The bound of tests/test_gpu_born.py::gn_against_backward."""
    s = sides[mode]
    pb, v = s.pb, s.vs[0]
    hip_ops.release()
    m = model(pb)
    hv = gn(hip_ops, pb, v, exact=False)
    jv = [d["ett"].cpu().numpy() for d in hip_ops.born(*m, *cuda(v), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])]
    bw = G.set_mode(pb, mode, name="bw_" + mode)
    hip_ops.obscalc(*m, pb["Stf"], 1, bw["Shot_ids"], bw["para_fname"])
    noise = 0.0
    for i, sid in enumerate(G.shots_of(pb)):
        syn = ft.read_shot_gather(bw["data_dir"], "ett", sid, pb["nSteps"])
        hip_ops.set_observed(bw["para_fname"], sid, torch.from_numpy((syn - jv[i]).astype(np.float32)))
        noise = max(noise, 1e-7 * float(np.abs(syn).max()) / float(np.abs(jv[i]).max()))
    g = [t.cpu().numpy() for t in hip_ops.backward(*m, pb["Stf"], 1, bw["Shot_ids"], bw["para_fname"])[1:4]]
    dev = []
    for name, a, b in zip(("hvLambda", "hvMu", "hvDen"), hv, g):
        assert np.isfinite(a).all() and np.abs(b).max() > 0
        dev.append(float(np.abs(a - b).max() / np.abs(b).max()))
        print("conditioned GN 4 %s %s: deviation from the gradient at obs = syn - J v %.2e of its maximum (bound %.2e = 10 x %.2e)" % (mode, name, dev[-1], 10 * noise, noise))
    assert max(dev) <= 10.0 * noise, (mode, dev, 10.0 * noise)


# ---- 5: the w mode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.MODES)
def test_w_mode_is_untouched_by_the_keys(hip_ops, sides, mode):
    """5: J^T w under the file, bit for bit J^T w under the same file without the keys (w stays in raw data space)."""
    s = sides[mode]
    pb, plain = s.pb, G.set_mode(s.pb, "none", name="plain_" + mode)
    w = [{"ett": torch.from_numpy(np.ascontiguousarray(g))} for g in s.jv[0][1]]
    got = [hip_ops.born_adjoint(*model(pb), w, pb["Stf"], 1, pb["Shot_ids"], p["para_fname"], with_source=True) for p in (pb, plain)]
    assert all(t.abs().max() > 0 for t in got[0])
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(*got))


# ---- 6: what stays refused --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["if_cross_misfit", "if_src_update"])
def test_the_other_two_keys_stay_refused(hip_ops, sides, key):
    """6: product, gradient and w mode of sepfwi_adjoint_exact and sepfwi_born with hv_*: -1, "conditioned" in the message, alone and on
    top of window and filter; the session serves the raw Born gathers afterwards, bit for bit the unconditioned ones -- as a linear file
    does."""
    from sepfwi import _native
    L = _native.lib()
    s = sides["both"]
    plain = G.set_mode(s.pb, "none", name="plain_" + key)
    m, v = model(s.pb), cuda(s.vs[0])
    stf, ids = s.pb["Stf"].contiguous(), np.ascontiguousarray(s.pb["Shot_ids"].numpy(), dtype=np.int32)
    n = sum(g.size for g in s.jv[0][0])
    w, g = torch.zeros(n, dtype=torch.float32, device="cuda"), [torch.zeros_like(m[0]) for _ in range(3)]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    raw = lambda pb: [d["ett"].cpu().numpy() for d in hip_ops.born(*m, *v, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])]
    base = raw(plain)
    assert all(np.abs(b).max() > 0 for b in base)
    for tag, mode in (("alone", "none"), ("on_both", "both")):
        pb = G.set_mode(s.pb, mode, name="%s_%s" % (key, tag), **{key: True})
        fn = pb["para_fname"].encode()

        def exact(w3=(None, None, None), v3=(None, None, None)):
            return L.sepfwi_adjoint_exact(None, *[p(t) for t in g], *[p(t) for t in w3], *[p(t) for t in v3], *[p(t) for t in m], p(stf), 0, int(ids.size),
                                          C.c_void_p(ids.ctypes.data), fn, None)

        for what, rc in (("product", exact(v3=v)), ("gradient", exact()), ("w", exact(w3=(w, None, None)))):
            msg = L.sepfwi_last_error()
            assert rc == -1 and b"conditioned" in msg and key.encode() in msg, (key, tag, what, rc, msg)
        rc = L.sepfwi_born(None, None, None, *[p(t) for t in g], *[p(t) for t in m], *[p(t) for t in v], p(stf), 0, int(ids.size), C.c_void_p(ids.ctypes.data), fn, None)
        assert rc == -1 and b"conditioned" in L.sepfwi_last_error() and key.encode() in L.sepfwi_last_error()
        assert all(np.array_equal(a, b) for a, b in zip(raw(pb), base)), (key, tag)
    assert all(np.array_equal(a, b) for a, b in zip(raw(s.pb), base)), "a linear file changed the raw Born gathers"


# ---- 7: edges ---------------------------------------------------------------------------------------------------------------------------
def thin(pb, shot, keep):
    """pb's survey with only the channels `keep` of one shot (the survey dict alone: set_mode writes the file)"""
    pb = dict(pb)
    sv = dict(pb["survey"])
    sh = dict(sv["shot%d" % shot])
    for k in ("z_rec", "x_rec"):
        sh[k] = [sh[k][i] for i in keep]
    sh["nrec"] = len(keep)
    sv["shot%d" % shot] = sh
    pb["survey"] = sv
    return pb


EDGES = ("window_error_1", "nrec_1", "ragged", "nsteps_odd")


@pytest.mark.parametrize("edge", EDGES)
def test_edges(tmp_path, oracle, oracle_nvfma, hip_ops, edge):
    """7: one channel whose window is empty ("Window error 1": its trace passes untouched); a shot with one channel; different channel
    counts over the two shots (an FFT plan each); an odd number of time steps -- v^T H v = |Z C J v|^2 of the exact product under window
    and filter, and sepfwi_condition against the oracle on the same gathers."""
    import problems as P
    pb = P.make_problem(str(tmp_path), **dict(G.SMALL, nSteps=121 if edge == "nsteps_odd" else G.SMALL["nSteps"]))
    if edge == "nrec_1":
        pb = thin(pb, 0, [pb["nrec"] // 2])
    if edge == "ragged":
        pb = thin(pb, 0, list(range(0, pb["nrec"], 3)))
    pb = G.set_mode(pb, "both", error1=(1, 5) if edge == "window_error_1" else None)
    s = Side(oracle, oracle_nvfma, pb, seeds=V_SEEDS[:1])
    if edge == "window_error_1":
        assert np.array_equal(G.C_of(oracle, G.set_mode(pb, "window", name="w_only", error1=(1, 5)), s.jv[0][0][1], 1)[5], s.jv[0][0][1][5])
    hip_ops.release()
    d = s.jv[0][0]
    got = unflat(hip_ops.condition(flat(d).cuda(), pb["Shot_ids"], pb["para_fname"]), d)
    for i, (x, r, a) in enumerate(zip(got, s.cjv[0][0], s.cjv[1][0])):
        top = float(np.abs(r).max())
        print("conditioned GN 7 %s shot %d (%d channels): C d against the oracle's, max-norm deviation %.2e of the maximum" % (edge, i, r.shape[0], float(np.abs(x - r).max()) / top))
        assert np.all(np.abs(x.astype(np.float64) - r) <= GATHER_TOL * top + 3.0 * np.abs(a.astype(np.float64) - r)), (edge, i)
    hv = gn(hip_ops, pb, s.vs[0])
    X.outside_is_zero(pb, hv, edge)
    held(X.model_dot(s.vs[0], hv), s.norm2(0), s.norm2(0, 1), "conditioned GN 7 %s v^T H v" % edge)


# ---- 8: the example -----------------------------------------------------------------------------------------------------------------------
def test_multiscale_example_with_gauss_newton(tmp_path, hip_ops):
    """8: examples/multiscale_fwi.py --gauss-newton at the size of tests/test_conditioning.py::test_multiscale_example_runs_band_by_band
    (two bands and the full band, 19 shots): every stage ends at a lower conditioned misfit than it began.  The default invocation prints the lines it printed: one per stage in the old format, then the recovery line."""
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("multiscale_fwi", os.path.join(ROOT, "examples", "multiscale_fwi.py"))
    ms = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ms)
    hip_ops.release()
    log, cur = ms.run(niter=1, n_bands=2, workdir=str(tmp_path / "gn"), verbose=False, gauss_newton=True, inner=2)
    assert [b for b, _, _ in log] == [ms.FILTER_TABLE[-2], ms.FILTER_TABLE[-1], None]
    for band, f0_, f1_ in log:
        print("conditioned GN 8 band %s: conditioned misfit %.6e -> %.6e" % (band, f0_, f1_))
        assert f1_ < f0_, (band, f0_, f1_)
    assert max(f for _, f, _ in log[:2]) < 1e-3 * log[2][1]      # (as in that test: a 10 Hz wavelet has little energy below 7.5 Hz)
    assert all(np.isfinite(c).all() for c in cur) and any(np.abs(c - c0).max() > 0 for c, c0 in zip(cur, (4000.0, 4000.0 / 1.732, 2500.0)))
    hip_ops.release()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        ms.run(niter=1, n_bands=1, workdir=str(tmp_path / "default"))
    lines = out.getvalue().strip().splitlines()
    num = r"-?\d\.\d{4}e[+-]\d\d"
    assert len(lines) == 3, lines
    assert re.fullmatch(r"stage 0, low-pass 2-7\.5 Hz: misfit %s -> %s in \d+ iterations \(\d+ evaluations\)" % (num, num), lines[0]), lines[0]
    assert re.fullmatch(r"stage 1, all frequencies: misfit %s -> %s in \d+ iterations \(\d+ evaluations\)" % (num, num), lines[1]), lines[1]
    assert re.fullmatch(r"recovered Vp anomaly peak -?\d+\.\d m/s \(true 80\), Vs -?\d+\.\d \(true -46\.2\), density -?\d+\.\d kg/m\^3 \(true 40\)", lines[2]), lines[2]
    hip_ops.release()
