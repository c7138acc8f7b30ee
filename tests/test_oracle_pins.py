"""Pins of the CPU oracles (CPU only).  The oracle is test infrastructure; these tests are what makes it
trustworthy:

  * oracle/numba_oracle.c   == the reference's own Python solver, bit for bit, on committed golden traces
    (generated in the build container by scripts/make_golden_numba.py, which imports
    DAS_Waveform_Modeling/src/elasticSolver.py from /root/reference);
  * numba oracle vs the reference's Aki-Richards analytic solution (peak-normalised, as the reference's
    notebook MNB/000-Solver-Benchmark.ipynb cells 12-13 compares them);
  * oracle/torchfwi_oracle.c (restatement of the CUDA path) vs the numba oracle: same operator sequence,
    amplitudes related by the source factors (SURVEY.md 8a "Equivalence note");
  * known answers printed by the reference's GPU runs: tests/test_known_answers.py.
"""
import os

import numpy as np
import pytest

import problems as P
from conftest import GOLDEN


def _run_numba(oracle, g, vp, vs, rho):
    return oracle.numba_forward(int(g["nx"]), int(g["nz"]), int(g["ndamp"]), float(g["dx"]), float(g["dz"]), float(g["dt"]),
                                int(g["nt"]), float(g["f0"]), vp, vs, rho, g["src_coord"], g["das_coord"], g["geo_coord"],
                                g["das_sensitivity"])


def test_numba_oracle_bit_exact_small(oracle):
    g = np.load(os.path.join(GOLDEN, "numba_small.npz"))
    sol = _run_numba(oracle, g, g["vp"], g["vs"], g["rho"])
    for i, s in enumerate(sol):
        for c in ("vx", "vz", "pr", "exx", "ezz", "exz", "ett"):
            assert np.array_equal(s[c], g["shot%d_%s" % (i, c)]), (i, c)


def test_numba_oracle_bit_exact_config1(oracle):
    """BASELINE.json configs[0]: 200x200 homogeneous, 1 Ricker shot, 500 steps."""
    g = np.load(os.path.join(GOLDEN, "numba_config1.npz"))
    n = (int(g["nx"]), int(g["nz"]))
    sol = _run_numba(oracle, g, np.full(n, float(g["vp0"])), np.full(n, float(g["vs0"])), np.full(n, float(g["rho0"])))[0]
    for c in ("vx", "vz", "pr", "exx", "ezz", "exz"):
        assert np.array_equal(sol[c], g[c]), c


def test_numba_oracle_vs_analytic(oracle):
    """configs[0] 'vs Aki-Richards analytic': peak-normalised velocity traces against the analytic 2-D
    displacement, exactly the comparison of the reference notebook (its wavelets differ by a time
    derivative pair, cell 15 of NB/000 notes this), tolerance: normalised RMS <= 5 % after the best
    integer-sample alignment (<= 2 samples)."""
    g = np.load(os.path.join(GOLDEN, "numba_config1.npz"))
    a = np.load(os.path.join(GOLDEN, "analytic_config1.npz"))
    src = a["src"]
    for r in (0, 1):
        rec = a["receivers"][r]
        sx, sz = np.sign(rec[0] - src[0]), np.sign(rec[1] - src[1])
        for comp, key, sg in (("vx", "rec%d_Ux" % r, sx), ("vz", "rec%d_Uz" % r, sz)):
            # analytic is evaluated for |offsets| (MNB/000 cell 8) and its sign convention is opposite to the
            # FD stress-source convention (the notebook multiplies by -1, MNB/000 cell 13; NB/000 cell 15)
            an = -a[key][:450] * sg
            fd = g[comp][r, :450]
            an = an / np.abs(an).max()
            fd = fd / np.abs(fd).max()
            best = min(np.sqrt(np.mean((np.roll(fd, s) - an) ** 2)) / np.sqrt(np.mean(an ** 2)) for s in range(-2, 3))
            assert best <= 0.05, (r, comp, best)


def test_torchfwi_oracle_matches_numba_oracle(oracle, tmp_path):
    """Homogeneous medium, early times (before the different absorbers matter): CUDA-order column k of
    vx, vz equals Numba column k times 1500^2*1e7*dt / (dt/2) = 4.5e13; ett = exx*dx times that; pressure
    column k+1 = 2 x Numba pr column k  (SURVEY.md 8a/8c-(i))."""
    n, npml, nt, dh, dt, f0 = 80, 20, 200, 10.0, 1.0e-3, 25.0
    pb = P.make_problem(str(tmp_path), nz=n, nx=n, nPml=npml, nSteps=nt, nshots=1, dh=dh, dt=dt, f0=f0, hetero=False,
                        src_z=40, src_x=[40], rec_z=30)
    sv = pb["survey"]["shot0"]
    lam, mu, den = pb["lame_init"]
    syn = oracle.cufd(lam.numpy(), mu.numpy(), den.numpy(), pb["Stf"].numpy(), 2, [0], pb["para"], pb["survey"])["syn"][0]
    vp = np.full((n, n), 3000.0)
    rec = np.stack([np.asarray(sv["x_rec"]) * dh, np.asarray(sv["z_rec"]) * dh], 1).astype(float)
    src = np.array([[sv["x_src"] * dh, sv["z_src"] * dh]], float)
    sens = np.zeros((rec.shape[0], 6)); sens[:, 0] = 1.0
    nb = oracle.numba_forward(n, n, npml, dh, dh, dt, nt, f0, vp, vp / 1.732, np.full((n, n), 2400.0), src, rec, rec, sens)[0]
    fac = 1500.0 ** 2 * 1.0e7 * dt / (dt / 2.0)
    early = 150      # direct arrivals only: absorber round trip (40 cells out, >= 30 back) arrives after 0.23 s
    near = np.abs(np.asarray(sv["x_rec"]) - sv["x_src"]) < 14
    assert near.sum() >= 10
    sel = np.where(near)[0]
    for comp, k, ref in (("vx", 1, nb["vx"] * fac), ("vz", 2, nb["vz"] * fac), ("ett", 3, nb["exx"] * dh * fac)):
        e = P.rel_l2(syn[k][sel, :early], ref[sel, :early])
        assert e <= 2e-3, (comp, e)
        # a one-sample misalignment would be an order of magnitude worse
        assert P.rel_l2(syn[k][sel, 1:early + 1], ref[sel, :early]) > 10 * max(e, 1e-4), comp
    e = P.rel_l2(syn[0][sel, 1:early + 1], 2.0 * nb["pr"][sel, :early] * fac)
    assert e <= 2e-3, ("pr", e)


@pytest.mark.parametrize("fiber", ["horizontal", "vertical"])
def test_oracle_axial_strain_is_the_one_cell_velocity_difference(oracle, tmp_path, fiber):
    """recording_exx / recording_ezz (Src/utilities.cu:593-602,620-629): along a fibre whose channels are one cell apart,
    channel r is exactly v_r - v_(r-1) of the along-fibre velocity component (not divided by the spacing)."""
    import problems as P
    pb = P.make_problem(str(tmp_path), hetero=True, nSteps=120, das_fiber=fiber)
    lam, mu, den = pb["lame_true"]
    syn = oracle.cufd(lam.numpy(), mu.numpy(), den.numpy(), pb["Stf"].numpy(), 2, pb["Shot_ids"].numpy(),
                      pb["para"], pb["survey"])["syn"]
    comp = 2 if fiber == "vertical" else 1     # vz : vx
    for i in range(syn.shape[0]):
        assert np.abs(syn[i, 3]).max() > 0
        assert np.array_equal(syn[i, 3][1:], syn[i, comp][1:] - syn[i, comp][:-1])


def test_oracle_vertical_fibre_gradient_is_consistent_with_finite_differences(oracle, tmp_path):
    """The vertical-fibre adjoint source (res_injection_ezz, Src/utilities.cu:632-641) is never launched by the reference,
    so there is no printed value to pin it on; check instead that <g, d> follows the misfit's directional derivative as
    closely as for the horizontal fibre (the reference adjoint is an approximate transpose)."""
    import problems as P
    out = {}
    for fiber in ("horizontal", "vertical"):
        pb = P.make_problem(str(tmp_path / fiber), hetero=False, nSteps=220, das_fiber=fiber, nshots=1, src_x=[20])
        lam_t, mu_t, den_t = [t.numpy() for t in pb["lame_true"]]
        lam, mu, den = [t.numpy() for t in pb["lame_init"]]
        args = (pb["Stf"].numpy(),)
        obs = oracle.cufd(lam_t, mu_t, den_t, *args, 2, pb["Shot_ids"].numpy(), pb["para"], pb["survey"])["syn"]
        r0 = oracle.cufd(lam, mu, den, *args, 1, pb["Shot_ids"].numpy(), pb["para"], pb["survey"], obs=obs)
        d = r0["gDen"] / np.abs(r0["gDen"]).max()
        eps = 2.0     # kg/m^3
        fp = oracle.cufd(lam, mu, den + eps * d, *args, 0, pb["Shot_ids"].numpy(), pb["para"], pb["survey"], obs=obs)["misfit"]
        fm = oracle.cufd(lam, mu, den - eps * d, *args, 0, pb["Shot_ids"].numpy(), pb["para"], pb["survey"], obs=obs)["misfit"]
        fd = (fp - fm) / (2 * eps)
        out[fiber] = (fd, float((r0["gDen"] * d).sum()))
    for fiber, (fd, gd) in out.items():
        assert abs(fd - gd) <= 0.05 * abs(gd), (fiber, fd, gd)


def test_long_run_golden_is_what_the_oracle_computes(tmp_path, oracle):
    """tests/golden/oracle_long4000.npz (4000 time steps; the GPU test compares against it) is the oracle's output on
    tests/problems.py LONG_RUN: same problem digest, same observed gather, same misfit and gradients, bit for bit."""
    import hashlib
    import problems as P
    G = np.load(os.path.join(GOLDEN, "oracle_long4000.npz"))
    pb = P.make_long_problem(str(tmp_path))
    h = hashlib.sha256()
    for t in list(pb["lame_true"]) + list(pb["lame_init"]) + [pb["Stf"]]:
        h.update(np.ascontiguousarray(t.numpy()).tobytes())
    assert h.hexdigest() == str(G["digest"])
    ids = pb["Shot_ids"].numpy()
    lam, mu, den = [t.numpy() for t in pb["lame_true"]]
    obs = oracle.cufd(lam, mu, den, pb["Stf"].numpy(), 2, ids, pb["para"], pb["survey"])["syn"]
    assert np.array_equal(obs[0, 3], G["obs_ett"])
    lam, mu, den = [t.numpy() for t in pb["lame_init"]]
    ref = oracle.cufd(lam, mu, den, pb["Stf"].numpy(), 1, ids, pb["para"], pb["survey"], obs=obs)
    n, nz, nx = pb["nPml"], P.LONG_RUN["nz"], P.LONG_RUN["nx"]
    assert ref["misfit"] == float(G["misfit"])
    for k in ("gLambda", "gMu", "gDen"):
        assert np.array_equal(ref[k][n:n + nz, n:n + nx + 1], G[k]), k
    assert np.array_equal(ref["gStf"][0], G["gStf"])


def test_directional_das_reduces_to_the_straight_fibres(oracle, tmp_path):
    """Survey key "das_sensitivity" (SURVEY.md 8f-3): with weight 1 on exx alone the directional channel IS recording_exx,
    with weight 1 on ezz alone it IS recording_ezz (Src/utilities.cu:593-602,620-629), observed data and gradients, bit
    for bit."""
    import problems as P
    for col, fiber in ((0, "horizontal"), (3, "vertical")):
        pb0 = P.make_problem(str(tmp_path / ("f" + fiber)), hetero=True, nSteps=150, das_fiber=fiber, nshots=1)
        nrec = pb0["nrec"]
        sens = np.zeros((nrec, 6)); sens[:, col] = 1.0
        sv = {k: (dict(v, das_sensitivity=sens.tolist()) if k.startswith("shot") and k != "nShots" and isinstance(v, dict) else v)
              for k, v in pb0["survey"].items()}
        para_h = dict(pb0["para"]); para_h.pop("das_fiber", None)
        lam_t, mu_t, den_t = [t.numpy() for t in pb0["lame_true"]]
        lam, mu, den = [t.numpy() for t in pb0["lame_init"]]
        stf, ids = pb0["Stf"].numpy(), pb0["Shot_ids"].numpy()
        obs0 = oracle.cufd(lam_t, mu_t, den_t, stf, 2, ids, pb0["para"], pb0["survey"])["syn"]
        obs1 = oracle.cufd(lam_t, mu_t, den_t, stf, 2, ids, para_h, sv)["syn"]
        assert np.array_equal(obs0, obs1), fiber
        g0 = oracle.cufd(lam, mu, den, stf, 1, ids, pb0["para"], pb0["survey"], obs=obs0)
        g1 = oracle.cufd(lam, mu, den, stf, 1, ids, para_h, sv, obs=obs1)
        for k in ("misfit", "gLambda", "gMu", "gDen", "gStf"):
            assert np.array_equal(g0[k], g1[k]), (fiber, k)


def test_directional_das_matches_the_numba_solver(oracle, tmp_path):
    """ett = s0 exx + s3 ezz + s1 exz (MOD/elasticSolver.py:266-276).  The Numba oracle is bit-exact to the reference's
    Python solver (golden ett traces, test_numba_oracle_bit_exact_small); here the CUDA-path oracle's directional channel,
    with random per-channel sensitivities, agrees with it on a homogeneous medium before the absorbers differ -- same
    comparison, factor 1500^2 1e7 dt / (dt/2) and strain x dx, as for the plain exx channel above."""
    n, npml, nt, dh, dt, f0 = 80, 20, 200, 10.0, 1.0e-3, 25.0
    rng = np.random.default_rng(5)
    pb = P.make_problem(str(tmp_path), nz=n, nx=n, nPml=npml, nSteps=nt, nshots=1, dh=dh, dt=dt, f0=f0, hetero=False,
                        src_z=40, src_x=[40], rec_z=30)
    nrec = pb["nrec"]
    sens = np.zeros((nrec, 6))
    sens[:, 0], sens[:, 3], sens[:, 1] = rng.uniform(-1, 1, nrec), rng.uniform(-1, 1, nrec), rng.uniform(-1, 1, nrec)
    sens[:, [2, 4, 5]] = rng.uniform(-1, 1, (nrec, 3))          # columns the 2-D solver ignores
    sv = dict(pb["survey"]); sv["shot0"] = dict(sv["shot0"], das_sensitivity=sens.tolist())
    lam, mu, den = pb["lame_init"]
    syn = oracle.cufd(lam.numpy(), mu.numpy(), den.numpy(), pb["Stf"].numpy(), 2, [0], pb["para"], sv)["syn"][0]
    s0 = sv["shot0"]
    vp = np.full((n, n), 3000.0)
    rec = np.stack([np.asarray(s0["x_rec"]) * dh, np.asarray(s0["z_rec"]) * dh], 1).astype(float)
    src = np.array([[s0["x_src"] * dh, s0["z_src"] * dh]], float)
    nb = oracle.numba_forward(n, n, npml, dh, dh, dt, nt, f0, vp, vp / 1.732, np.full((n, n), 2400.0), src, rec, rec, sens)[0]
    fac = 1500.0 ** 2 * 1.0e7 * dt / (dt / 2.0)
    early = 150
    sel = np.where(np.abs(np.asarray(s0["x_rec"]) - s0["x_src"]) < 14)[0]
    ref = nb["ett"] * dh * fac
    e = P.rel_l2(syn[3][sel, :early], ref[sel, :early])
    assert e <= 2e-3, e
    # each strain component on its own (sensitivity 1 on one column) -- catches a swapped column or staggering
    for col, key in ((0, "exx"), (3, "ezz"), (1, "exz")):
        one = np.zeros((nrec, 6)); one[:, col] = 1.0
        sv1 = dict(pb["survey"]); sv1["shot0"] = dict(sv["shot0"], das_sensitivity=one.tolist())
        s1 = oracle.cufd(lam.numpy(), mu.numpy(), den.numpy(), pb["Stf"].numpy(), 2, [0], pb["para"], sv1)["syn"][0]
        e = P.rel_l2(s1[3][sel, :early], nb[key][sel, :early] * dh * fac)
        assert e <= 3e-3, (key, e)
        assert P.rel_l2(s1[3][sel, 1:early + 1], nb[key][sel, :early] * dh * fac) > 10 * max(e, 1e-4), key


def test_directional_das_gradient_is_consistent_with_finite_differences(oracle, tmp_path):
    """The directional adjoint source is the transpose of the directional recording: <g, d> follows the misfit's
    directional derivative as closely as the reference's own exx channel does (homogeneous background)."""
    pb = P.make_problem(str(tmp_path), hetero=False, nSteps=220, nshots=1, src_x=[20], das_sensitivity="random")
    lam_t, mu_t, den_t = [t.numpy() for t in pb["lame_true"]]
    lam, mu, den = [t.numpy() for t in pb["lame_init"]]
    stf, ids = pb["Stf"].numpy(), pb["Shot_ids"].numpy()
    obs = oracle.cufd(lam_t, mu_t, den_t, stf, 2, ids, pb["para"], pb["survey"])["syn"]
    r0 = oracle.cufd(lam, mu, den, stf, 1, ids, pb["para"], pb["survey"], obs=obs)
    d = r0["gDen"] / np.abs(r0["gDen"]).max()
    eps = 2.0
    fp = oracle.cufd(lam, mu, den + eps * d, stf, 0, ids, pb["para"], pb["survey"], obs=obs)["misfit"]
    fm = oracle.cufd(lam, mu, den - eps * d, stf, 0, ids, pb["para"], pb["survey"], obs=obs)["misfit"]
    fd, gd = (fp - fm) / (2 * eps), float((r0["gDen"] * d).sum())
    assert abs(fd - gd) <= 0.05 * abs(gd), (fd, gd)


@pytest.mark.parametrize("case", ["stride3", "vertical", "directional", "bandpass", "gauge4"])
def test_headline_receivers_goldens_match_their_problems(tmp_path, case):
    """tests/golden/oracle_headline_receivers_<case>.npz (the GPU test tests/test_gpu_headline.py::test_headline_grid_general_receivers
    compares against them) belong to the problems scripts/make_golden_headline_receivers.py builds today: same input digest (models,
    source function, survey, parameter file), same seam and windows, source and channels where the generator says.  A drift of
    tests/problems.py fails here, on the CPU, instead of first on the GPU.  The oracle is not run (4e9 cell-updates a case)."""
    import scripts.make_golden_headline_receivers as mg
    path = mg.golden_path(case)
    assert os.path.getsize(path) < 1 << 20
    G = np.load(path)
    pb = mg.make_case(str(tmp_path), case)
    assert mg.digest(pb) == str(G["digest"]), "problem generator drifted: regenerate with scripts/make_golden_headline_receivers.py"
    assert pb["nSteps"] == G["gStf"].shape[0] == mg.NSTEPS
    nzc = pb["nz_pad"] - pb["nPad"]
    assert nzc == 1064 and pb["nx_pad"] == 2064
    seam = int(G["seam"])
    assert seam == pb["seam"] == round(mg.SEAM_BAND * nzc / mg.NBAND)
    sh = pb["survey"]["shot0"]
    n = pb["nPml"]
    assert 0 < seam - (int(sh["z_src"]) + n) <= 2                          # the source just above the seam
    z_rec = np.asarray(sh["z_rec"]) + n
    if case == "vertical":
        assert z_rec.min() < seam <= z_rec.max() and abs(int(sh["x_src"]) - int(sh["x_rec"][0])) == 20
    else:
        assert np.all(z_rec == seam)                                       # the line on the first row below it
    assert "filter" in pb["para"] if case == "bandpass" else "filter" not in pb["para"]
    assert pb["para"].get("das_gauge_length") == (mg.GAUGE * pb["para"]["dx"] if case == "gauge4" else None)
    for w in ("win_src", "win_seam"):
        assert tuple(int(v) for v in G[w]) == pb[w]
        z0, z1, x0, x1 = pb[w]
        assert 0 <= z0 < z1 <= nzc and 0 <= x0 < x1 <= pb["nx_pad"] and G["gMu_" + w].shape == (z1 - z0, x1 - x0)
    assert G["gLambda_dec"].shape == (-(-pb["nz_pad"] // mg.DECIM), -(-pb["nx_pad"] // mg.DECIM))
    assert G["res_energy"].shape == (pb["nrec"],) and G["obs_ett"].shape == (G["channels"].size, pb["nSteps"])
