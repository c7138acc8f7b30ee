"""The yardstick of the fan-filter tests (tests/fk_ref.py), checked on the CPU alone.  fk_ref states the definition of the stage through the
full complex fft2 in float64; here: its output is real, the operator is symmetric, reject = 1 - pass, C^T = Wn . B . FK transposes
C = FK . B . Wn, it separates two plane waves of opposite apparent slowness, the Nyquist rule is what makes the first two hold, and the
inputs of the pass-level GPU test (tests/test_gpu_fk_passes.py) feel the stage.  This licenses the yardstick; the tests that fail without
the feature are tests/test_fk_config.py, tests/test_gpu_fk_data.py and tests/test_gpu_fk_passes.py.

Bounds.
  imaginary part, symmetry, reject = 1 - pass   1e-12: float64 transforms of at most 256 x 1200 points carry eps log2(N) = 4e-15.
  transpose of the chain                        1e-9 of |C a| |b|: the oracle's window and band-pass hand on float32 arrays, each rounding
                                                3.4e-8 rms of an element, which a dot product over N = 77 400 elements averages to
                                                3.4e-8 / sqrt(N) = 1.2e-10 per rounding, two roundings a side.
  plane waves                                   kept energy >= 0.99, rejected <= 1e-3, on the central half of the channels.
  Nyquist rule dropped                          imaginary part or asymmetry above 1e-6 on at least one size.
  pass-level inputs                             | |C_fk d| / |C d| - 1 | > 0.10 for every J v and the residual (cond_gn_ref: inputs_discriminate).

Measured: the module prints every figure before it asserts; profiles/r32_fk_filter.txt keeps them."""
import numpy as np
import pytest

import cond_gn_ref as G
import data_entry_common as DC
import exact_adjoint_ref as X
import fk_ref as F

TIGHT, CHAIN_TOL = 1e-12, 1e-9
CORNERS = (-2e-4, 1e-4, 6e-4, 9e-4)      # an asymmetric band with zero on a ramp
DT, DELTA = 1e-3, 10.0


def _pair(nrec, nt, seed=0):
    rng = np.random.default_rng(seed + 1000 * nrec + nt)
    return rng.standard_normal((nrec, nt)), rng.standard_normal((nrec, nt))


def _sym(fa, a, fb, b):
    return abs(float((fa * b).sum()) - float((a * fb).sum())) / float(np.sqrt((fa ** 2).sum() * (b ** 2).sum()))


@pytest.mark.parametrize("reject", [False, True])
@pytest.mark.parametrize("size", F.SIZES)
def test_the_stage_is_real_symmetric_and_reject_complements_pass(size, reject):
    a, b = _pair(*size)
    fa, ia = F.fk_full(a, DT, DELTA, CORNERS, reject)
    fb, ib = F.fk_full(b, DT, DELTA, CORNERS, reject)
    other = F.fk(a, DT, DELTA, CORNERS, not reject)
    comp = float(np.abs(fa + other - a).max() / np.abs(a).max())
    ratio = float(np.linalg.norm(fa) / np.linalg.norm(a))
    print("fk reference %s %s: imaginary part %.2e / %.2e of the real one, asymmetry %.2e, |pass + reject - 1| %.2e, |FK d| / |d| %.3f"
          % (size, "reject" if reject else "pass", ia, ib, _sym(fa, a, fb, b), comp, ratio))
    assert max(ia, ib) <= TIGHT and _sym(fa, a, fb, b) <= TIGHT and comp <= TIGHT
    assert 0.05 < ratio < 0.98      # it does something, and not everything


def test_a_band_with_p2_equal_to_p3_is_served():
    a, b = _pair(33, 65)
    c = (1e-4, 3e-4, 3e-4, 7e-4)
    fa, ia = F.fk_full(a, DT, DELTA, c)
    fb, _ = F.fk_full(b, DT, DELTA, c)
    assert ia <= TIGHT and _sym(fa, a, fb, b) <= TIGHT and np.isfinite(fa).all() and np.linalg.norm(fa) > 0
    assert float(F.trapezoid(np.array([3e-4]), c)[0]) == 1.0


def test_without_the_nyquist_rule_the_output_is_complex_or_the_operator_asymmetric():
    worst = 0.0
    for size in F.SIZES:
        a, b = _pair(*size)
        fa, ia = F.fk_full(a, DT, DELTA, CORNERS, nyquist=False)
        fb, _ = F.fk_full(b, DT, DELTA, CORNERS, nyquist=False)
        print("fk reference, Nyquist rule dropped, %s: imaginary part %.2e, asymmetry %.2e" % (size, ia, _sym(fa, a, fb, b)))
        worst = max(worst, ia, _sym(fa, a, fb, b))
    assert worst > 1e-6


def test_two_plane_waves_are_separated():
    up, down = F.plane_waves()
    c = (1e-4, 2e-4, 6e-4, 8e-4)
    mid = slice(16, 48)
    kept = float((F.fk(up, DT, DELTA, c)[mid] ** 2).sum() / (up[mid] ** 2).sum())
    left = float((F.fk(down, DT, DELTA, c)[mid] ** 2).sum() / (down[mid] ** 2).sum())
    rej = float((F.fk(up, DT, DELTA, c, reject=True)[mid] ** 2).sum() / (up[mid] ** 2).sum())
    print("fk reference, plane waves p = +-4e-4 s/m, band %s: energy kept of +p %.5f, left of -p %.2e; reject mode leaves %.2e of +p" % (c, kept, left, rej))
    assert kept >= 0.99 and left <= 1e-3 and rej <= 1e-3
    # the sign of p: with p = +k / f the band would keep the other event
    assert float((F.fk(down, DT, DELTA, tuple(-v for v in c[::-1]))[mid] ** 2).sum() / (down[mid] ** 2).sum()) >= 0.99


def test_spacing_follows_the_survey():
    para = dict(dz=5.0, dx=10.0)
    sv = lambda z, x: {"shot0": dict(nrec=len(z), z_rec=z, x_rec=x)}
    assert F.spacing(para, sv([3, 3, 3], [4, 5, 6]), 0) == 10.0
    assert F.spacing(para, sv([3, 4, 5], [4, 4, 4]), 0) == 5.0
    assert F.spacing(para, sv([3, 3, 3], [4, 7, 10]), 0) == 30.0
    assert abs(F.spacing(para, sv([3, 5, 7], [9, 8, 7]), 0) - np.hypot(10.0, 10.0)) < 1e-12
    for z, x in (([3], [4]), ([3, 3, 3], [4, 5, 7]), ([3, 3], [4, 4])):
        with pytest.raises(ValueError, match="fk_slowness"):
            F.spacing(para, sv(z, x), 0)


@pytest.mark.parametrize("mode", ["pass", "reject"])
def test_ct_is_the_transpose_of_c_under_filter_window_and_fan(oracle, tmp_path, mode):
    keys = {"filter": [25.0, 60.0, 260.0, 400.0], "if_win": True, "fk_slowness": [-2e-4, 1e-4, 6e-4, 9e-4], "fk_mode": mode}
    pb = DC.problem(tmp_path, 600, (64, 65), keys, "fkref", misfit_key=None, nx=80)
    a, b = DC.traces(pb, 1), DC.traces(pb, 2)
    ca = G.C_all(oracle, pb, a, F.C_of)
    lhs, rhs = G.dot(ca, b), G.dot(a, G.C_all(oracle, pb, b, F.Ct_of))
    gap = abs(lhs - rhs) / (G.norm(ca) * G.norm(b))
    wrong = abs(lhs - G.dot(a, G.C_all(oracle, pb, b, F.C_of))) / (G.norm(ca) * G.norm(b))      # C^T with the stages in C's order
    print("fk reference, chain %s: <C a, b> %.8e, <a, C^T b> %.8e, gap %.2e of |C a| |b|; with C in the place of C^T %.2e" % (mode, lhs, rhs, gap, wrong))
    assert G.norm(ca) > 0 and gap <= CHAIN_TOL
    assert wrong > 1e3 * CHAIN_TOL


def test_the_pass_level_inputs_feel_the_fan(oracle, tmp_path):
    """inputs_discriminate for tests/test_gpu_fk_passes.py: every J v it uses (smooth_v seeds 3 and 4) and its residual lose or gain more
    than 10 % in norm through the fan on top of C = B . Wn -- a pass that leaves the stage out, or applies it on one side only, shows."""
    pb = F.pass_problem(tmp_path)
    obs, _ = G.oracle_gathers(oracle, pb, "lame_true")
    syn, _ = G.oracle_gathers(oracle, pb, "lame_init")
    gathers = {"J v (3)": G.jv_ett(oracle, pb, X.smooth_v(pb, 3)), "J u (4)": G.jv_ett(oracle, pb, X.smooth_v(pb, 4)),
               "obs - syn": [o.astype(np.float64) - s for o, s in zip(obs, syn)], "syn": syn}
    for name, d in gathers.items():
        with_fk, without = G.norm(G.C_all(oracle, pb, d, F.C_of)), G.norm(G.C_all(oracle, pb, d, G.C_of))
        per_shot = [G.norm([F.C_of(oracle, pb, g, s)]) / G.norm([G.C_of(oracle, pb, g, s)]) for g, s in zip(d, G.shots_of(pb))]
        print("fk pass-level inputs, %s: |C_fk d| %.4e, |C d| %.4e, ratio %.3f (per shot %s)" % (name, with_fk, without, with_fk / without, ["%.3f" % r for r in per_shot]))
        assert without > 0 and abs(with_fk / without - 1.0) > 0.10, name
