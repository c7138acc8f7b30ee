"""The reference of the normalised cross-correlation misfit (tests/cross_ref.py), licensed on the CPU: the adjoint source is minus the
derivative of the misfit through the oracle's whole float32 conditioning chain (central differences, the bound 2e-3 of
tests/test_conditioning.py); the misfit does not see a positive factor on the synthetics and the adjoint source is orthogonal to them,
trace by trace; dead traces give the values the definition gives; the float32 restatement of the same expressions
(oracle.conditioned_residual, what the suite's other cross-correlation tests compare with) is NOT this reference on nearly fitting data --
so the GPU comparison can fail; and the seeded inputs of tests/test_gpu_cross_data.py are what they were.

Measured here:
  whole chain     central differences against -<a, d syn>: 1.0e-6 ... 2.1e-5 of the derivative at the better of two steps (bound 2e-3)
  invariance      f(obs, k syn) - f(obs, syn), k = 0.37 ... 1e3: up to 1.0e-11 sum |w| (nSteps 2; 7e-14 at 257), and 1.1e-6 at k = 1e-3, where
                  DIVCONST / n_ss is 1e6 times larger; <a_r, s_r>: up to 1.1e-11 w_r (bounds: 4 DIVCONST / min n + 1e-13)
  float32 restatement against this reference, adjoint source rel-L2, obs = c syn + eta noise on the band-limited traces of the GPU test,
  5 and 257 channels, nSteps 65, 257, 600, the key alone / if_win / filter (float64 transforms on both sides):
      eta 1      5e-8 ... 2e-7          eta 1e-2   7e-7 ... 1e-5          eta 1e-3   1e-5 ... 1.2e-4          eta 1e-4   8e-5 ... 1.0e-3
  at c = -2, eta 1e-4: 6.1e-4 ... 1.0e-3; the pinned input (5 channels, nSteps 257, the key alone): 8.4e-4, 8.4 x the GPU test's 1e-4.
  Its misfit stays within 1.3 x 2^-24 sum |w| everywhere: the cancellation is in the adjoint source alone.
profiles/r24_cross_and_source_update_data.txt holds the figures of one run."""
import hashlib
import json

import numpy as np
import pytest
import torch

import cond_gn_ref as G
import cross_ref as X
import data_entry_common as DC

DATA_TOL = 1e-4                        # tests/test_gpu_cross_data.py's
INPUTS_DIGEST = "25131d87104b099d95cc1dccd11b12ad2cc027efee3213ef1e62a41deda89227"


def rnd(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


# ---- the whole float32 chain ----------------------------------------------------------------------------------------------------------------
def chain_problem(mode):
    """the sizes, windows and weights of tests/test_conditioning.py::test_conditioned_adjoint_source_against_finite_differences as a
    one-shot pb under the key"""
    rng = np.random.default_rng(11)
    nrec, nt, dt = 5, 400, 2.0e-3
    t = np.arange(nt) * dt
    mk = lambda: (np.exp(-((t - 0.4) / 0.15) ** 2)[None] * np.sin(2 * np.pi * rng.uniform(8, 20, (nrec, 1)) * t[None] + rng.uniform(0, 6, (nrec, 1)))).astype(np.float32)
    obs, syn = mk(), mk()
    sh = dict(nrec=nrec, win_start=list(rng.uniform(0.05, 0.2, nrec)), win_end=list(rng.uniform(0.5, 0.75, nrec)), weights=list(rng.uniform(0.5, 2.0, nrec)), src_weight=1.3)
    para = {"dt": dt, X.KEY: True}
    if mode in ("window", "both"):
        para["if_win"] = True
    if mode in ("filter", "both"):
        para["filter"] = [3.0, 6.0, 30.0, 45.0]
    d = mk() * 0.5
    d[:, 0] = 0.0
    return dict(para=para, survey={"shot0": sh}, Shot_ids=torch.zeros(1, dtype=torch.int32)), obs, syn, d


@pytest.mark.parametrize("mode", ["none", "window", "filter", "both"])
def test_adjoint_source_is_minus_the_derivative_through_the_oracle_chain(oracle, mode):
    """d misfit = -<a, d syn> with a = C^T [w (o - (n_os / n_ss) s) / (|o| |s|)] through the oracle's float32 window and band-pass: central
    differences with the step 1e-2 of tests/test_conditioning.py and with 1e-3, the better of the two, to that test's 2e-3."""
    pb, obs, syn, d = chain_problem(mode)
    f0, a, wsum = X.data_misfit(oracle, pb, [obs], [syn])
    an = -float((a[0].astype(np.float64) * d).sum())
    gap = {}
    for eps in (1e-2, 1e-3):
        fp = X.data_misfit(oracle, pb, [obs], [(syn + eps * d).astype(np.float32)])[0]
        fm = X.data_misfit(oracle, pb, [obs], [(syn - eps * d).astype(np.float32)])[0]
        fd = (fp - fm) / (2 * eps)
        gap[eps] = abs(fd - an) / max(abs(fd), abs(an))
    cosine = abs(an) / float(np.linalg.norm(a[0]) * np.linalg.norm(d))
    print("cross ref chain %s: misfit %.8e (sum |w| %.4f), -<a, d> %.8e (cosine %.3f), gap of the central difference by step %s"
          % (mode, f0, wsum, an, cosine, {k: "%.2e" % v for k, v in gap.items()}))
    assert abs(f0) < wsum and cosine > 1e-2 and min(gap.values()) <= 2e-3, (mode, an, gap)
    # and the float32 restatement is the same function on such (far from fitting) data
    f32, a32 = X.float32_restatement(oracle, pb, [obs], [syn])
    assert abs(f32 - f0) <= 16 * 2.0 ** -24 * wsum and DC.rel(a32, a) <= 1e-5


# ---- invariance -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [2, 3, 60, 257])
def test_misfit_is_scale_invariant_and_the_adjoint_source_orthogonal_to_the_synthetics(nt):
    """With C the identity: f(obs, k syn) = f(obs, syn) for k > 0 and <a_r, s_r> = 0 for every trace -- exactly so without DIVCONST, and
    with it to DIVCONST / n: the traces are scaled to norms n >= 20, and both bounds are stated in the misfit's own unit, the weights, as
    4 DIVCONST / min n (+ 1e-13 of float64 rounding) of them -- |a_r| |s_r| would not do: it vanishes where obs is parallel to syn."""
    nrec = 4
    o, s = 10.0 * rnd(nt, nrec, nt).astype(np.float64) + 8.0, 10.0 * rnd(nt + 1, nrec, nt).astype(np.float64) - 8.0
    w = np.array([0.7, 0.0, 1.9, 1.2])
    n_oo, n_ss, _ = X.norms(o, s)
    bound = 4.0 * X.DIVCONST / float(min(n_oo.min(), n_ss.min())) + 1e-13
    f = X.misfit(o, s, w)
    for k in (1e-3, 0.37, 2.0, 1e3):
        fk = X.misfit(o, k * s, w)
        print("cross ref nt %d: f(obs, %g syn) - f(obs, syn) = %.2e of sum |w|" % (nt, k, abs(fk - f) / w.sum()))
        assert abs(fk - f) <= (bound * max(1.0, 1.0 / k ** 2)) * w.sum()   # DIVCONST / n_ss grows with 1 / k^2
    a = X.adjoint_source(o, s, w)
    for r in range(nrec):
        gap = abs(float((a[r] * s[r]).sum()))     # = w DIVCONST |n_os / n_ss - 1| / (|o| |s|) <= 2 w DIVCONST / min n: of the misfit's own unit, w
        print("cross ref nt %d trace %d: <a, s> = %.2e (w %.1f, |a| |s| %.2e)" % (nt, r, gap, w[r], float(np.linalg.norm(a[r]) * np.linalg.norm(s[r]))))
        assert (np.linalg.norm(a[r]) > 0) == (w[r] != 0) and gap <= bound * w[r]
    assert min(n_oo.min(), n_ss.min()) >= 20.0 and X.misfit(o, o, w) == pytest.approx(-w.sum(), abs=1e-12)


# ---- dead traces ----------------------------------------------------------------------------------------------------------------------------
def test_dead_traces_give_finite_and_defined_values():
    """DIVCONST is what defines a dead trace: obs = 0 gives cc = sqrt(DIVCONST) / |s| and a = -w DIVCONST s / (n_ss sqrt(DIVCONST) |s|);
    syn = 0 gives the same cc with |o| and a = w o / (|o| sqrt(DIVCONST)); both zero give cc = 1 (DIVCONST / DIVCONST) and a = 0."""
    nt = 50
    x = rnd(3, 1, nt)[0].astype(np.float64)
    zero = np.zeros(nt)
    o, s = np.stack([zero, x, zero, x]), np.stack([x, zero, zero, 0.5 * x])
    w = np.array([1.5, 0.8, 1.1, 2.0])
    c, a = X.cc(o, s), X.adjoint_source(o, s, w)
    nx, rd = float((x * x).sum()) + X.DIVCONST, np.sqrt(X.DIVCONST)
    print("cross ref dead traces: cc %s, |a| %s" % (c, np.linalg.norm(a, axis=1)))
    assert np.isfinite(c).all() and np.isfinite(a).all()
    assert c[0] == pytest.approx(rd / np.sqrt(nx), rel=1e-12) and c[1] == pytest.approx(rd / np.sqrt(nx), rel=1e-12)
    assert c[2] == 1.0 and not a[2].any() and c[3] == pytest.approx(1.0, abs=1e-9)
    np.testing.assert_allclose(a[0], -w[0] * (X.DIVCONST / nx) * x / (rd * np.sqrt(nx)), rtol=1e-12, atol=0)
    np.testing.assert_allclose(a[1], w[1] * x / (np.sqrt(nx) * rd), rtol=1e-12, atol=0)
    assert X.misfit(o, s, w) == pytest.approx(-float((w * c).sum()), rel=1e-15)


# ---- the comparison can fail ----------------------------------------------------------------------------------------------------------------
def near_fit_problem(tmp, nt=257, nrec=(5,), keys=None):
    pb = DC.problem(tmp, nt, nrec, keys or {}, "near", misfit_key=X.KEY)
    return pb, DC.traces(pb, 2), DC.traces(pb, 5)


def test_the_float32_restatement_misses_the_reference_on_nearly_fitting_data(oracle, tmp_path):
    """On obs = -2 syn + 1e-4 noise (five channels, 257 steps, the key alone: an input of tests/test_gpu_cross_data.py) the adjoint source of
    oracle.conditioned_residual(..., cross=True) -- the same expressions with float32 norms and a float32 difference -- is off this
    reference by 8.4e-4 rel-L2: at least 5 x the 1e-4 the GPU test allows, so a kernel that keeps float32 there fails it.  At eta = 1 the
    two agree to 1e-7, and the misfit agrees throughout."""
    pb, syn, noise = near_fit_problem(tmp_path)
    dev = {}
    for eta in (1.0, 1e-2, 1e-3, 1e-4):
        obs = X.near_fit(syn, noise, -2.0, eta)
        f, a, wsum = X.data_misfit(oracle, pb, obs, syn)
        f32, a32 = X.float32_restatement(oracle, pb, obs, syn)
        dev[eta] = DC.rel(a32, a)
        print("cross ref float32 restatement, c -2, eta %.0e: adjoint source rel-L2 %.2e off the float64 reference (|a| %.4e), misfit gap %.2f x 2^-24 sum |w|"
              % (eta, dev[eta], G.norm(a), abs(f32 - f) / (2.0 ** -24 * wsum)))
        assert G.norm(a) > 0 and abs(f32 - f) <= 16 * 2.0 ** -24 * wsum
    assert dev[1.0] <= 1e-6 and dev[1e-4] >= 5 * DATA_TOL, dev


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------------------
def test_inputs_of_the_gpu_tests_are_what_they_were(tmp_path):
    """The survey (windows, weights) and the seeded traces that tests/test_gpu_cross_data.py and tests/test_gpu_source_update_data.py draw,
    and one nearly fitting gather, hash to the digest taken when they were written."""
    h = hashlib.sha256()
    for nt, nrec in ((65, (5, 3)), (257, (5,)), (3, (1,))):
        pb = DC.problem(tmp_path / ("d%d" % nt), nt, nrec, {}, "digest", misfit_key=X.KEY)
        h.update(json.dumps({k: {q: v[q] for q in ("nrec", "win_start", "win_end", "weights", "src_weight")} for k, v in sorted(pb["survey"].items()) if k.startswith("shot")}, sort_keys=True).encode())
        syn, noise = DC.traces(pb, 2), DC.traces(pb, 5, amp=1e-3)
        for g in syn + noise + X.near_fit(syn, noise, 0.37, 1e-2):
            assert g.dtype == np.float32
            h.update(np.ascontiguousarray(g).tobytes())
    assert h.hexdigest() == INPUTS_DIGEST, h.hexdigest()
