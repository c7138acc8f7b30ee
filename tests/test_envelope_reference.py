"""The reference of the envelope misfit (tests/envelope_ref.py), licensed on the CPU: the Hilbert transform is antisymmetric and D^T the
transpose of D; the adjoint source is minus the derivative of the misfit (central differences in float64, then through the oracle's whole
float32 conditioning chain, then through the propagator); the Gauss-Newton operator is the Hessian where the residual vanishes; the
misfit does not cycle-skip where the L2 misfit does; and the inputs that the GPU tests reuse discriminate.

Measured here (float64 unless said):
  antisymmetry      <Hx, y> + <x, Hy>  0 ... 9e-17 of |Hx| |y|;  <D d, w> - <d, D^T w>  7e-18 ... 6e-17 of |D d| |w|   (nt 2, 3, 60, 257)
  first derivative  1.1e-4, 1.1e-6, 1.1e-8, 1.1e-10 of |D^T rho| |d| at steps 1e-2 ... 1e-5: 100 per decade (a quartic)
  Gauss-Newton      second central difference at obs = syn against |Z D d|^2: 5.7e-8 relative at step 1e-4
  whole chain       float32 oracle chain: 2e-8 ... 9e-6 of the derivative at the better of two steps (bound 2e-3, tests/test_conditioning.py's)
  propagation       50 x 90 heterogeneous problem: 3.6e-2, 4.2e-4, 1.1e-4 at steps 10, 1, 0.1 (bound 1e-3 at the best rung)
profiles/r21_envelope_misfit.txt holds the figures of one run."""
import numpy as np
import pytest

import born_ref as B
import cond_gn_ref as G
import envelope_ref as E
from fuzz_common import GRAD_TOL

NTS = (2, 3, 60, 257)


def rnd(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


# ---- antisymmetry -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", NTS)
def test_hilbert_is_antisymmetric_and_dt_the_transpose_of_d(nt):
    x, y, s, d, w = (rnd(k + 10 * nt, 3, nt) for k in range(5))
    hx, hy = E.hilbert(x), E.hilbert(y)
    gap = abs(float((hx * y).sum() + (x * hy).sum()))
    scale = float(np.linalg.norm(hx) * np.linalg.norm(y))
    print("envelope ref nt %d: <Hx, y> + <x, Hy> = %.2e of |Hx| |y|" % (nt, gap / scale))
    assert scale > 0 and gap <= 1e-12 * scale
    dd, dtw = E.D(s, d), E.Dt(s, w)
    lhs, rhs = float((dd * w).sum()), float((d * dtw).sum())
    scale = float(np.linalg.norm(dd) * np.linalg.norm(w))
    print("envelope ref nt %d: <D d, w> %.12e, <d, D^T w> %.12e, gap %.2e of |D d| |w|" % (nt, lhs, rhs, abs(lhs - rhs) / scale))
    assert scale > 0 and abs(lhs - rhs) <= 1e-12 * scale
    # The Nyquist bin of a real trace is real, so -i times it is purely imaginary, and a complex-to-real inverse transform ignores the
    # imaginary part of that bin: keeping the bin changes nothing.  Zeroing it states what the transform computes.
    assert np.array_equal(E.hilbert(x, keep_nyquist=True), hx)


# ---- first derivative -------------------------------------------------------------------------------------------------------------------
def test_adjoint_source_is_minus_the_derivative():
    """-<D^T rho, d> against central differences of the misfit along d, steps 1e-2 ... 1e-5: the misfit is a quartic in the data, so the
    deviation is h^2 f''' / 6 exactly and falls by 100 per decade; it reaches 1e-6 of |D^T rho| |d|.  (The bound is stated against
    |D^T rho| |d|: the directional derivative of random traces is a small fraction of it.)"""
    nt = 400
    o = np.stack([E.wavelet(nt, shift=0.0), E.wavelet(nt, shift=0.01, f=22.0)]).astype(np.float32)
    s = np.stack([E.wavelet(nt, shift=0.02), E.wavelet(nt, shift=-0.015, f=18.0)]).astype(np.float32)
    d = rnd(5, 2, nt).astype(np.float64)
    a = E.adjoint_source(o, s)
    an = -float((a * d).sum())
    scale = float(np.linalg.norm(a) * np.linalg.norm(d))
    devs = []
    for h in (1e-2, 1e-3, 1e-4, 1e-5):
        fd = (E.misfit(o, s + h * d) - E.misfit(o, s - h * d)) / (2.0 * h)
        devs.append(abs(fd - an) / scale)
        print("envelope ref first derivative, step %.0e: finite difference %.10e, -<D^T rho, d> %.10e, deviation %.2e of |D^T rho| |d| (%.2e of the derivative)"
              % (h, fd, an, devs[-1], abs(fd - an) / abs(an)))
    assert abs(an) > 1e-3 * scale
    for p, q in zip(devs[:-1], devs[1:]):
        assert 50.0 <= p / q <= 200.0, devs
    assert devs[-1] <= 1e-6, devs


# ---- Gauss-Newton -------------------------------------------------------------------------------------------------------------------------
def test_gauss_newton_is_the_hessian_where_the_residual_vanishes():
    nt = 400
    s = np.stack([E.wavelet(nt, shift=0.02), E.wavelet(nt, shift=-0.015, f=18.0)]).astype(np.float32)
    d = rnd(6, 2, nt).astype(np.float64)
    h = 1e-4
    second = (E.misfit(s, s + h * d) - 2.0 * E.misfit(s, s) + E.misfit(s, s - h * d)) / (h * h)
    zd = E.Z(E.D(s, d))
    ref = float((zd * zd).sum())
    quad = float((d * E.gn(s, d)).sum())
    print("envelope ref Gauss-Newton: second difference %.10e, |Z D d|^2 %.10e (gap %.2e), <d, D^T Z D d> %.10e (gap %.2e)"
          % (second, ref, abs(second - ref) / ref, quad, abs(quad - ref) / ref))
    assert E.misfit(s, s) == 0.0 and abs(second - ref) <= 1e-6 * ref and abs(quad - ref) <= 1e-12 * ref
    u = rnd(7, 2, nt).astype(np.float64)
    sym = float((u * E.gn(s, d)).sum()) - float((d * E.gn(s, u)).sum())
    assert abs(sym) <= 1e-12 * ref


# ---- the whole float32 chain ----------------------------------------------------------------------------------------------------------------
def chain_problem(mode):
    """the sizes and windows of tests/test_conditioning.py::test_conditioned_adjoint_source_against_finite_differences as a one-shot pb.  Its
    gathers share ONE Gaussian envelope and differ in the carrier alone -- the envelope misfit of such a pair is zero, which is its point --
    so the Gaussians here differ in centre and width from gather to gather and trace to trace."""
    rng = np.random.default_rng(11)
    nrec, nt, dt = 5, 400, 2.0e-3
    t = np.arange(nt) * dt
    mk = lambda: (np.exp(-((t[None] - rng.uniform(0.3, 0.5, (nrec, 1))) / rng.uniform(0.1, 0.2, (nrec, 1))) ** 2)
                  * np.sin(2 * np.pi * rng.uniform(8, 20, (nrec, 1)) * t[None] + rng.uniform(0, 6, (nrec, 1)))).astype(np.float32)
    obs, syn = mk(), mk()
    sh = dict(nrec=nrec, win_start=list(rng.uniform(0.05, 0.2, nrec)), win_end=list(rng.uniform(0.5, 0.75, nrec)), weights=list(rng.uniform(0.5, 2.0, nrec)), src_weight=1.3)
    para = {"dt": dt, E.KEY: True}
    if mode in ("window", "both"):
        para["if_win"] = True
    if mode in ("filter", "both"):
        para["filter"] = [3.0, 6.0, 30.0, 45.0]
    d = mk() * 0.5
    d[:, 0] = 0.0
    import torch
    return dict(para=para, survey={"shot0": sh}, Shot_ids=torch.zeros(1, dtype=torch.int32)), obs, syn, d


@pytest.mark.parametrize("mode", ["none", "window", "filter", "both"])
def test_adjoint_source_through_the_whole_oracle_chain(oracle, mode):
    """d misfit = -<a, d syn> with a = C^T D^T rho through the oracle's float32 window and band-pass, as
    tests/test_conditioning.py checks the other misfits of the same chain, with its bound 2e-3.  Central differences with that test's step
    1e-2 and with 1e-3, the better of the two (the truncation error of a quartic, h^2 f''' / 6, falls by 100 from the one to the other, the
    float32 chain's rounding rises by 10): measured 2e-8 ... 9e-6."""
    pb, obs, syn, d = chain_problem(mode)
    f0, a, rhos, dts = E.data_misfit(oracle, pb, [obs], [syn])
    an = -float((a[0].astype(np.float64) * d).sum())
    gap = {}
    for eps in (1e-2, 1e-3):
        fp = E.data_misfit(oracle, pb, [obs], [(syn + eps * d).astype(np.float32)])[0]
        fm = E.data_misfit(oracle, pb, [obs], [(syn - eps * d).astype(np.float32)])[0]
        fd = (fp - fm) / (2 * eps)
        gap[eps] = abs(fd - an) / max(abs(fd), abs(an))
    cosine = abs(an) / float(np.linalg.norm(a[0]) * np.linalg.norm(d))
    print("envelope ref chain %s: misfit %.6e, -<a, d> %.8e (cosine %.3f), gap of the central difference by step %s" % (mode, f0, an, cosine, {k: "%.2e" % v for k, v in gap.items()}))
    assert f0 > 0 and cosine > 1e-2 and min(gap.values()) <= 2e-3, (mode, an, gap)
    # the Gauss-Newton operator of the chain: symmetric, and its quadratic form the norm of Z D C d
    u = np.roll(d, 7, axis=1) * 0.7
    gd, gu = E.data_gn(oracle, pb, [syn], [d]), E.data_gn(oracle, pb, [syn], [u])
    zd = E.zdc(oracle, pb, [syn], [d])
    q, ref = G.dot([d], gd), G.dot(zd, zd)
    print("envelope ref chain %s: <d, GN d> %.8e, |Z D C d|^2 %.8e (gap %.2e); <u, GN d> - <d, GN u> %.2e of it"
          % (mode, q, ref, abs(q - ref) / ref, abs(G.dot([u], gd) - G.dot([d], gu)) / ref))
    assert abs(q - ref) <= 1e-4 * ref and abs(G.dot([u], gd) - G.dot([d], gu)) <= 1e-4 * ref


# ---- through the propagator -------------------------------------------------------------------------------------------------------------------
def test_gradient_direction_against_finite_differences_of_the_oracle(oracle, tmp_path):
    """The 50 x 90 heterogeneous problem of tests/test_born_reference.py under the key with a band-pass: central differences of the
    envelope misfit of the oracle's gathers along a smooth model perturbation v against -<a, J v>, J v from born_ref; the best rung of
    a decade ladder within the suite's gradient tolerance 1e-3."""
    pb, _ = B.water_problem(tmp_path, "A")
    pb = dict(pb, para=dict(pb["para"], **{E.KEY: True, "filter": G.corners(float(pb["para"]["f0"]))}))
    v = B.perturbation(pb)
    obs, _ = G.oracle_gathers(oracle, pb, "lame_true")
    syn, _ = G.oracle_gathers(oracle, pb, "lame_init")
    f0, a, _, _ = E.data_misfit(oracle, pb, obs, syn)
    an = -G.dot(a, G.jv_ett(oracle, dict(pb, para=E.plain_para(pb)), v))
    m = [t.numpy() for t in pb["lame_init"]]
    plain, stf, ids = E.plain_para(pb), pb["Stf"].numpy(), pb["Shot_ids"].numpy()
    gap = {}
    for eps in (10.0, 1.0, 0.1):
        e = np.float32(eps)
        f = []
        for sign in (1.0, -1.0):
            g = oracle.cufd(*[x + np.float32(sign) * e * y for x, y in zip(m, v)], stf, 2, ids, plain, pb["survey"])["syn"]
            f.append(E.data_misfit(oracle, pb, obs, [g[i][B.ROW["ett"]] for i in range(len(ids))])[0])
        gap[eps] = abs((f[0] - f[1]) / (2.0 * eps) - an) / abs(an)
    print("envelope ref propagation: misfit %.6e, -<a, J v> %.8e, gap of the central difference by step %s" % (f0, an, {k: "%.2e" % x for k, x in gap.items()}))
    assert f0 > 0 and min(gap.values()) <= GRAD_TOL, gap


# ---- cycle skipping ---------------------------------------------------------------------------------------------------------------------------
def test_envelope_misfit_does_not_cycle_skip_where_l2_does():
    """a 20 Hz wavelet under a Gaussian of 80 ms, shifted 0 ... 75 ms (1.5 periods): the envelope misfit grows monotonically, the L2
    misfit has a second minimum at one period (50 ms)."""
    nt = 400
    o = E.wavelet(nt)[None]
    shifts = np.arange(0, 76, 5) * 1e-3
    env = [E.misfit(o, E.wavelet(nt, shift=s)[None]) for s in shifts]
    l2 = [0.5 * float((E.Z(o - E.wavelet(nt, shift=s)[None]) ** 2).sum()) for s in shifts]
    print("envelope ref cycle skipping: shift [ms] %s\n  envelope %s\n  L2       %s" % ([int(round(s * 1e3)) for s in shifts], ["%.3e" % x for x in env], ["%.3e" % x for x in l2]))
    assert env[0] == 0.0 and all(b > a for a, b in zip(env[:-1], env[1:]))
    k = int(np.argmin(np.abs(shifts - 0.05)))
    assert l2[k] < l2[k - 2] and l2[k] < l2[k + 2] and l2[k] < 0.5 * max(l2)


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", list(E.KEYSETS))
def test_inputs_of_the_gpu_tests_discriminate(oracle, tmp_path, keys):
    """So that the GPU comparison cannot pass vacuously: the envelope gradient differs from the L2 gradient of the same file by rel-L2
    > 0.05 in every parameter, and the Hilbert term 2 H((H s) rho) is at least 0.1 of |D^T rho| in every shot."""
    pb = E.gpu_problem(tmp_path, keys)
    obs, full = G.oracle_gathers(oracle, pb, "lame_true")
    syn, _ = G.oracle_gathers(oracle, pb, "lame_init")
    f, a, rhos, dts = E.data_misfit(oracle, pb, obs, syn)
    for i, sid in enumerate(G.shots_of(pb)):
        cs = E.C_of(oracle, pb, syn[i], sid)
        part = float(np.linalg.norm(E.hilbert_term(cs, rhos[i])) / np.linalg.norm(dts[i]))
        print("envelope inputs %s shot %d: |2 H((H s) rho)| = %.3f |D^T rho|" % (keys, sid, part))
        assert part >= 0.1
    g_env = E.gradient(oracle, pb, a)
    l2_para = {k: v for k, v in pb["para"].items() if k != E.KEY}
    g_l2 = oracle.cufd(*[t.numpy() for t in pb["lame_init"]], pb["Stf"].numpy(), 1, pb["Shot_ids"].numpy(), l2_para, pb["survey"], obs=np.stack(full))
    for name in ("gLambda", "gMu", "gDen"):
        x, y = g_env[name].astype(np.float64), g_l2[name].astype(np.float64)
        x, y = x / np.linalg.norm(x), y / np.linalg.norm(y)
        gap = float(np.linalg.norm(x - y))
        print("envelope inputs %s %s: normalised envelope gradient against the normalised L2 gradient, rel-L2 %.3f (misfit %.4e)" % (keys, name, gap, f))
        assert gap > 0.05
