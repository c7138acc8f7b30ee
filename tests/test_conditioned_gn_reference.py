"""The yardstick of the conditioned Gauss-Newton tests (tests/cond_gn_ref.py), checked on the CPU alone: C = band-pass . window of the
oracle is what "band-pass, then window" transposes, and -<Z C J v, Z (C obs - C syn)> with J from tests/born_ref.py is the directional
derivative of the oracle's own conditioned misfit (oracle.cufd with the keys).  This licenses the yardstick; the tests that fail without
the feature are in tests/test_gpu_conditioned_gauss_newton.py.

Bounds.
  symmetry       |<C a, b> - <a, C^T b>| <= 1e-5 |C a| |b|, float64 accumulation.  Both sides are float32 arrays that went through two
                 transforms of length 2 nSteps = 240: eps log2(240) = 5e-7 per transform in single precision (the nvfma build), two a side;
                 the bound is 5 x that.  The window is pointwise and exact.
  linearisation  best of the decade ladder of tests/test_born_reference.py within 3 x 2.66e-4 = 8e-4 of the analytic value, relative:
                 the agreement that file reports (and asserts, with the same 3 x) for the unconditioned axial strain of the joint v.

Measured (small problem 40 x 48, 120 steps, two shots; v = smooth 3; the three linear modes of cond_gn_ref and its narrow band):
  symmetry, gap / (|C a| |b|)   plain build: filter 8.4e-10, window 4.5e-10, both 1.2e-10, narrow 1.9e-10
                                nvfma build: filter 1.9e-10, window 4.5e-10, both 3.4e-10, narrow 1.1e-09
  linearisation, relative deviation of the central difference by eps (10, 1, 0.1, 0.01, 0.001):
            filter  4.1e+00 4.0e-02 1.9e-04 5.6e-04 1.4e-02
            window  3.7e+00 3.7e-02 1.3e-04 8.1e-05 2.2e-02
            both    4.7e+00 4.7e-02 2.6e-04 5.6e-04 1.7e-02
            narrow  4.2e+00 4.2e-02 2.1e-04 5.9e-04 1.4e-02
  (truncation ~ eps^2 above the minimum -- the record ends inside the first arrival, whose time shift with the model is a large
  second-order term -- and the round-off of a float32 misfit ~ 1 / eps below it)"""
import numpy as np
import pytest

import cond_gn_ref as G
import exact_adjoint_ref as X

SYM_TOL = 1e-5
LADDER = (10.0, 1.0, 0.1, 0.01, 0.001)      # tests/test_born_reference.py
FD_LEVEL = 2.66e-4                          # ... its MEASURED[("A", None)] for the axial strain, asserted there with the factor 3


@pytest.fixture(scope="module")
def problems(tmp_path_factory):
    return {mode: G.linear_problem(tmp_path_factory.mktemp("cgn_ref_" + mode), mode) for mode in G.ALL_MODES}


@pytest.mark.parametrize("mode", G.ALL_MODES)
def test_band_pass_then_window_is_the_transpose_of_c(oracle, oracle_nvfma, problems, mode):
    pb = problems[mode]
    rng = np.random.default_rng(11)
    shape = [(int(pb["survey"]["shot%d" % s]["nrec"]), pb["nSteps"]) for s in G.shots_of(pb)]
    a = [rng.standard_normal(s).astype(np.float32) for s in shape]
    b = [rng.standard_normal(s).astype(np.float32) for s in shape]
    for name, lib in (("plain", oracle), ("nvfma", oracle_nvfma)):
        ca = G.C_all(lib, pb, a)
        lhs, rhs = G.dot(ca, b), G.dot(a, G.C_all(lib, pb, b, G.Ct_of))
        gap = abs(lhs - rhs) / (G.norm(ca) * G.norm(b))
        print("conditioned GN reference, symmetry %s on the %s build: <C a, b> %.8e, <a, C^T b> %.8e, gap %.2e of |C a| |b|" % (mode, name, lhs, rhs, gap))
        assert G.norm(ca) > 0 and gap <= SYM_TOL, (mode, name, gap)
    wrong = G.dot(a, G.C_all(oracle, pb, b))      # C in the place of C^T: what the symmetry check must be able to see, where the two differ
    if mode == "both":
        assert abs(G.dot(G.C_all(oracle, pb, a), b) - wrong) / (G.norm(G.C_all(oracle, pb, a)) * G.norm(b)) > 100 * SYM_TOL


@pytest.mark.parametrize("mode", G.ALL_MODES)
def test_conditioned_misfit_is_linearised_by_z_c_j(oracle, problems, mode):
    pb = problems[mode]
    v = X.smooth_v(pb, 3)
    jv = G.jv_ett(oracle, pb, v)
    cjv = G.inputs_discriminate(oracle, pb, jv, "reference, " + mode)
    obs, obs_full = G.oracle_gathers(oracle, pb, "lame_true")
    syn, _ = G.oracle_gathers(oracle, pb, "lame_init")
    r, mis = G.conditioned_residual(oracle, pb, obs, syn)
    analytic = -G.dot([G.Z(c) for c in cjv], r)
    m = [t.numpy() for t in pb["lame_init"]]
    stf, ids = pb["Stf"].numpy(), pb["Shot_ids"].numpy()
    full = np.stack(obs_full)

    def misfit(eps):
        return oracle.cufd(*[a + np.float32(eps) * b for a, b in zip(m, v)], stf, 0, ids, pb["para"], pb["survey"], obs=full)["misfit"]

    m0 = misfit(0.0)
    print("conditioned GN reference, %s: misfit of oracle.cufd %.8e, 1/2 |Z (C obs - C syn)|^2 %.8e" % (mode, m0, mis))
    assert abs(m0 - mis) <= 1e-6 * mis      # (the same numpy chain, float32 storage of the residual against float64)
    dev = {}
    for eps in LADDER:
        fd = (misfit(eps) - misfit(-eps)) / (2.0 * eps)
        dev[eps] = abs(fd - analytic) / abs(analytic)
    print("conditioned GN reference, %s: -<Z C J v, Z (C obs - C syn)> = %.8e; relative deviation of the central difference by eps: %s"
          % (mode, analytic, {e: "%.2e" % d for e, d in dev.items()}))
    assert analytic != 0.0 and min(dev.values()) <= 3.0 * FD_LEVEL, (mode, dev)
