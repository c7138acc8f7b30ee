"""The normalised cross-correlation misfit's kernels alone, on the GPU (-m gpu), with no time loop: k_normfact, k_cross_misfit and
k_cross_adjoint through fwi_ops.data_misfit under if_cross_misfit, on seeded band-limited traces, against tests/cross_ref.py (float64 on
float32 inputs; C and C^T the oracle's; tests/test_cross_reference.py licenses it and shows that the float32 restatement the suite's other
cross-correlation tests compare with would not do here).

Shapes: nSteps 2, 3 (one and two live samples: obs is parallel to syn there, the hardest cancellation), 63, 64, 65 (a wavefront of the
per-trace reduction), 255, 256, 257 (its block) and 600; one channel, five, two shots with 5 and 3 (a plan per trace count), and -- at
nSteps 65 and 257, on a grid wide enough to hold them -- 64, 65, 257 channels and two shots with 513 and 2: k_cross_misfit sums the channels
with 256 threads and a stride loop.  Key sets: the key alone (C: the end taper, w = 1), with filter, with if_win (channel 1 has weight 0,
the last channel of a shot with three or more an empty window), with both.  Trace amplitudes 1 and 1e-3: DIVCONST is absolute.

Tolerances, none new: the adjoint source to rel-L2 1e-4, the seismogram tolerance of the other data-space tests; the misfit within
16 x 2^-24 sum_r |w_r| of the reference, absolute -- a term w_r n_os / (sqrt(n_oo) sqrt(n_ss)) goes through about eleven float32
roundings (three norms, two roots, a product, a quotient, the weight's product, the sum, the halving, the float32 result) and is at most
|w_r|; the value sits near -sum w, so a relative 1e-4 would test nothing.  Nearly fitting data, obs = c syn + eta noise, are the cases the
kernels were rewritten for (norms kept in double, obs - (n_os / n_ss) syn formed in double and rounded once): with float32 norms the
pointwise cases at eta = 1e-4 miss the 1e-4 by 1.9 ... 5.7 x, and nSteps 2 by everything
(profiles/r24_cross_and_source_update_data.txt).  Under filter two float32 conditioned gathers are subtracted and a float32 transform
carries its own noise into the residual, so eta is 1 and 1e-2 there and the
bound is 1e-4 + 3 x the distance between the reference evaluated with the oracle's float64 transforms and with its single-precision
build -- the two-roundings yardstick of the suite; it has to stay below 1e-2 of the reference.  Every comparison prints its deviation
before it asserts.

Measured on the MI355X: misfit within 1.02 x 2^-24 sum |w|; adjoint source within 2.7e-7 on independent traces (0 at nSteps 2), 6.4e-8
on pointwise nearly fitting data at every eta, 3.1e-5 under filter at eta 1e-2 where the two transforms differ by 2.7e-5; every live trace
of the dead-trace cases within 2.9e-7 of itself."""
import numpy as np
import pytest
import torch

import cond_gn_ref as G
import cross_ref as X
import data_entry_common as DC
from data_entry_common import flat, rel, traces, unflat

pytestmark = pytest.mark.gpu
DATA_TOL, MISFIT_ULPS, YARD, LIVE = 1e-4, 16, 3.0, 1e-2
LAYOUTS = {"one": (1,), "five": (5,), "ragged": (5, 3)}
WIDE = {"w64": (64,), "w65": (65,), "w257": (257,), "w513_2": (513, 2)}      # nSteps 65 and 257 only
WIDE_NX = 560
FILTER = [25.0, 60.0, 260.0, 400.0]      # tests/test_gpu_envelope_data.py's: the traces carry 25 ... 175 Hz, the lower ramp cuts into them
KEYSETS = {"alone": {}, "filter": {"filter": FILTER}, "window": {"if_win": True}, "both": {"filter": FILTER, "if_win": True}}
CASES = [(nt, name) for name in LAYOUTS for nt in DC.NSTEPS] + [(nt, name) for name in WIDE for nt in (65, 257)]


def problem(tmp, nt, layout, keys, name):
    wide = layout in WIDE
    return DC.problem(tmp, nt, (WIDE if wide else LAYOUTS)[layout], KEYSETS[keys], name, misfit_key=X.KEY, nx=WIDE_NX if wide else 48)


def run(hip_ops, pb, obs, syn):
    f, a = hip_ops.data_misfit(flat(obs).cuda(), flat(syn).cuda(), pb["Shot_ids"], pb["para_fname"])
    return f, unflat(a, obs)


def misfit_bound(wsum):
    return MISFIT_ULPS * 2.0 ** -24 * wsum


# ---- against the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt,layout", CASES)
def test_data_misfit_against_the_reference(oracle, hip_ops, tmp_path, nt, layout):
    for keys in KEYSETS:
        hip_ops.release()
        pb = problem(tmp_path / keys, nt, layout, keys, "cross")
        for amp in (1.0, 1e-3):
            obs, syn = traces(pb, 1, amp), traces(pb, 2, amp)
            f_ref, a_ref, wsum = X.data_misfit(oracle, pb, obs, syn)
            f, a = run(hip_ops, pb, obs, syn)
            dev = (abs(f - f_ref), rel(a, a_ref))
            print("cross data nt %d %s %s amplitude %g: misfit %.8e (reference %.8e, gap %.2e = %.2f x 2^-24 sum |w|, sum |w| %.4f), adj rel-L2 %.2e (|a| %.4e)"
                  % (nt, layout, keys, amp, f, f_ref, dev[0], dev[0] / (2.0 ** -24 * wsum), wsum, dev[1], G.norm(a_ref)))
            assert wsum > 0 and G.norm(a_ref) > 0
            assert dev[0] <= misfit_bound(wsum) and dev[1] <= DATA_TOL, (nt, layout, keys, amp, dev)
    hip_ops.release()


# ---- dead traces ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", list(KEYSETS))
def test_dead_traces(oracle, hip_ops, tmp_path, keys):
    """Five channels, 257 steps: channel 0 dead in both gathers (cc = DIVCONST / DIVCONST = 1, a = 0), channel 2 dead in obs, channel 3 dead
    in syn (a = w o / (|o| sqrt(DIVCONST)), 3e4 times a live trace's).  The adjoint source is compared TRACE BY TRACE, each to 1e-4 of the
    reference's trace: the rel-L2 of the gather would see channel 3 alone."""
    hip_ops.release()
    pb = problem(tmp_path, 257, "five", keys, "dead")
    for amp in (1.0, 1e-3):
        obs, syn = traces(pb, 1, amp), traces(pb, 2, amp)
        obs[0][0] = 0.0
        syn[0][0] = 0.0
        obs[0][2] = 0.0
        syn[0][3] = 0.0
        f_ref, a_ref, wsum = X.data_misfit(oracle, pb, obs, syn)
        f, a = run(hip_ops, pb, obs, syn)
        print("cross data dead traces %s amplitude %g: misfit %.8e (reference %.8e, gap %.2f x 2^-24 sum |w|)" % (keys, amp, f, f_ref, abs(f - f_ref) / (2.0 ** -24 * wsum)))
        assert np.isfinite(f) and np.isfinite(a[0]).all() and abs(f - f_ref) <= misfit_bound(wsum)
        live = 0
        for r in range(5):
            n_ref = float(np.linalg.norm(a_ref[0][r].astype(np.float64)))
            gap = float(np.linalg.norm(a[0][r].astype(np.float64) - a_ref[0][r]))
            print("cross data dead traces %s amplitude %g channel %d: |a| %.4e, gap %.2e of it" % (keys, amp, r, n_ref, gap / n_ref if n_ref else 0.0))
            if n_ref == 0.0:      # both dead, or weight 0
                assert not a[0][r].any()
            else:
                live += 1
                assert gap <= DATA_TOL * n_ref, (keys, amp, r)
        assert not a[0][0].any() and live >= 3
    hip_ops.release()


# ---- nearly fitting data ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["five", "w257"])
@pytest.mark.parametrize("nt", [65, 257, 600])
def test_nearly_fitting_data(oracle, oracle_nvfma, hip_ops, tmp_path, nt, layout):
    """obs = c syn + eta noise, c in {1, 0.37, -2}: what every late iteration of an inversion looks like.  Pointwise conditioning (the key
    alone, if_win): eta 1e-2, 1e-3, 1e-4 to the plain 1e-4.  Under filter: eta 1 and 1e-2, to 1e-4 + 3 x the two transforms' distance."""
    for keys in KEYSETS:
        hip_ops.release()
        pb = problem(tmp_path / keys, nt, layout, keys, "near")
        syn, noise = traces(pb, 2), traces(pb, 5)
        filtered = "filter" in KEYSETS[keys]
        for c in (1.0, 0.37, -2.0):
            for eta in ((1.0, 1e-2) if filtered else (1e-2, 1e-3, 1e-4)):
                obs = X.near_fit(syn, noise, c, eta)
                f_ref, a_ref, wsum = X.data_misfit(oracle, pb, obs, syn)
                yard = 0.0
                if filtered:
                    yard = rel(X.data_misfit(oracle_nvfma, pb, obs, syn)[1], a_ref)
                f, a = run(hip_ops, pb, obs, syn)
                dev = (abs(f - f_ref), rel(a, a_ref))
                print("cross data near fit nt %d %s %s c %g eta %.0e: misfit gap %.2f x 2^-24 sum |w|, adj rel-L2 %.2e (|a| %.4e, two transforms %.2e, bound %.2e)"
                      % (nt, layout, keys, c, eta, dev[0] / (2.0 ** -24 * wsum), dev[1], G.norm(a_ref), yard, DATA_TOL + YARD * yard))
                assert G.norm(a_ref) > 0 and yard < LIVE
                assert dev[0] <= misfit_bound(wsum) and dev[1] <= DATA_TOL + YARD * yard, (nt, layout, keys, c, eta, dev, yard)
    hip_ops.release()


# ---- pointers and repeatability -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", ["alone", "both"])
def test_host_and_device_pointers_and_a_second_call_give_the_same_bits(hip_ops, tmp_path, keys):
    from sepfwi import _native
    hip_ops.release()
    pb = problem(tmp_path, 257, "ragged", keys, "bits")
    obs, syn = flat(traces(pb, 1)), flat(traces(pb, 2))
    keep = [t.clone() for t in (obs, syn)]
    fd, ad = hip_ops.data_misfit(obs.cuda(), syn.cuda(), pb["Shot_ids"], pb["para_fname"])
    fh, ah = hip_ops.data_misfit(obs, syn, pb["Shot_ids"], pb["para_fname"])
    f2, a2 = hip_ops.data_misfit(obs.cuda(), syn.cuda(), pb["Shot_ids"], pb["para_fname"])
    assert ad.is_cuda and not ah.is_cuda and ad.abs().max() > 0
    assert fd == fh == f2 and torch.equal(ad.cpu(), ah) and torch.equal(ad, a2)
    assert all(torch.equal(a, b) for a, b in zip(keep, (obs, syn))), "an input was changed"
    with pytest.raises(_native.SepFwiError) as e:
        hip_ops.data_gn(syn.cuda(), obs.cuda(), pb["Shot_ids"], pb["para_fname"])
    assert e.value.code == -1 and "if_cross_misfit" in str(e.value)
    hip_ops.release()
