"""The reference that the geophone GPU tests rest on (tests/geophone_ref.py), checked on the CPU: with weights (1, 0, 0) the Python step
driver IS the oracle, bit for bit, for every fibre kind; its per-component sums are the oracle's residuals squared and summed; and its
gradient with vx / vz weights is the gradient of the weighted misfit (finite differences)."""
import numpy as np
import pytest

import geophone_ref as G
import problems as P


def _problem(tmp_path, **kw):
    opts = dict(nz=50, nx=90, nPml=10, nSteps=260, nshots=1, hetero=True, rec_z=30)
    opts.update(kw)
    pb = P.make_problem(str(tmp_path), **opts)
    lam, mu, den = pb["lame_init"]
    pb["lame_init"] = ((lam * 1.05).contiguous(), mu, den)      # residuals of the size of the data
    return pb


def _fiber_kw(fiber):
    return dict(das_fiber="vertical") if fiber == "vertical" else dict(das_sensitivity="random", nrec_stride=2) if fiber == "directional" else {}


@pytest.mark.parametrize("fiber", ["horizontal", "vertical", "directional"])
def test_driver_with_default_weights_is_the_oracle(oracle, tmp_path, fiber):
    """Weights (1, 0, 0): gLambda, gMu, gDen, gStf and all four gathers equal oracle.cufd's bit for bit (two shots: also the reduction
    over shots); the per-component sums equal the oracle's residuals, squared and summed in float64."""
    pb = _problem(tmp_path, nshots=2, nSteps=150, **_fiber_kw(fiber))
    stf, ids = pb["Stf"].numpy(), pb["Shot_ids"].numpy()
    obs = oracle.cufd(*[t.numpy() for t in pb["lame_true"]], stf, 2, ids, pb["para"], pb["survey"])["syn"]
    init = [t.numpy() for t in pb["lame_init"]]
    plain = oracle.cufd(*init, stf, 1, ids, pb["para"], pb["survey"], obs=obs, want_residual=True)
    ref = G.cufd(oracle, *init, stf, 1, ids, pb["para"], pb["survey"], obs=obs)
    assert np.abs(plain["gMu"]).max() > 0 and np.abs(plain["gStf"]).max() > 0
    for k in ("gLambda", "gMu", "gDen", "gStf", "syn"):
        assert np.array_equal(ref[k], plain[k]), k
    sums = (plain["res"].astype(np.float64) ** 2).sum((0, 2, 3))
    for k, name in ((1, "vx"), (2, "vz"), (3, "ett")):
        assert sums[k] > 0 and ref["parts"][name] == 0.5 * sums[k], name
    assert abs(ref["misfit"] - plain["misfit"]) <= 1e-6 * plain["misfit"]      # float64 sum here, the reference's float32 tree there


@pytest.mark.parametrize("weights", [(0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.5, 2.0)], ids=["vx", "vz", "joint"])
def test_geophone_gradient_is_consistent_with_finite_differences(oracle, tmp_path, weights):
    """<gDen, d> against central finite differences of the weighted misfit along the normalised density gradient, eps = 2 kg/m^3, as
    the gauge and vertical-fibre checks do it and with their bound, 5 % (the reference's adjoint is an approximate transpose).
    Homogeneous model: on the heterogeneous one the plain axial-strain channel itself is at 7 %."""
    pb = _problem(tmp_path, hetero=False)
    stf, ids = pb["Stf"].numpy(), pb["Shot_ids"].numpy()
    obs = oracle.cufd(*[t.numpy() for t in pb["lame_true"]], stf, 2, ids, pb["para"], pb["survey"])["syn"]
    lam, mu, den = [t.numpy() for t in pb["lame_init"]]
    r0 = G.cufd(oracle, lam, mu, den, stf, 1, ids, pb["para"], pb["survey"], obs=obs, weights=weights)
    assert r0["misfit"] > 0 and np.abs(r0["gDen"]).max() > 0

    def misfit(den_):
        return G.cufd(oracle, lam, mu, den_, stf, 0, ids, pb["para"], pb["survey"], obs=obs, weights=weights)["misfit"]

    d = r0["gDen"] / np.abs(r0["gDen"]).max()
    eps = 2.0     # kg/m^3
    fd = (misfit(den + eps * d) - misfit(den - eps * d)) / (2 * eps)
    gd = float((r0["gDen"].astype(np.float64) * d).sum())
    print("geophone finite differences, weights %r: fd %.6e, <g, d> %.6e, deviation %.2e" % (weights, fd, gd, abs(fd - gd) / abs(gd)))
    assert abs(fd - gd) <= 0.05 * abs(gd), (weights, fd, gd)
