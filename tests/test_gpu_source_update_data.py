"""The source-signature update's kernels alone, on the GPU (-m gpu), with no time loop: k_matching_coef, k_apply_coef and the two
Conditioner calls around them (source_update, source_update_adj) through fwi_ops.data_misfit under if_src_update, against
oracle.conditioned_residual(..., src_update=True) -- the numpy restatement that tests/test_conditioning.py licenses (a matching filter,
its adjoint step the exact transpose, the adjoint source against finite differences).

Shapes: the nSteps of tests/data_entry_common.py; one channel, five, two shots with 5 and 3, and -- at nSteps 65 and 257, on a grid wide
enough to hold them -- 257 channels and two shots with 513 and 2: k_matching_coef sums the channels with 256 threads and a stride loop.
Key sets: the key alone, with filter, with filter and if_win.  Inputs: independent traces, and obs = syn convolved with a two-tap
wavelet plus 1e-2 noise, which the update nearly fits.

Trace amplitudes 1 and 1e-3: the 1e-6 that damps the spectral division is absolute.  At amplitude 1 it is 1e-7 of sum |C_r|^2 and
invisible; at 1e-3 it is of that sum's size and a tenth of the data stays in the residual.  A SINGLE channel runs at 1e-3 alone: one
coefficient per frequency fits one channel exactly, whatever the traces, so at amplitude 1 its residual is what rounding leaves -- the
oracle's own two builds then differ by up to 0.27 in the misfit and 0.14 of the adjoint source (nSteps 2 with filter and if_win; 2e-2 ...
6e-2 at 255 ... 600), and the comparison would have no target.  At 1e-3 the damped residual is the target, and the two builds agree to
1.5e-5 or better in every case (5e-8 ... 1.5e-5 of the adjoint source, 1.7e-6 of the misfit).  That one channel IS fitted at amplitude 1
is test_one_channel_without_noise_is_fitted.

Tolerances: the misfit to the suite's 1e-4, relative; the adjoint source to rel-L2 1e-4 + 3 x the distance between the oracle's two
transform builds (float64 / single precision: the two-roundings yardstick of the suite), which has to stay below 1e-2 of the
reference.  Every comparison prints its deviation before it asserts; profiles/r24_cross_and_source_update_data.txt holds the figures
measured on the MI355X: misfit within 2.4e-6 (the oracle's two builds: 2.3e-6), adjoint source within 1.9e-5 (two builds: 1.7e-5)."""
import numpy as np
import pytest
import torch

import cond_gn_ref as G
import data_entry_common as DC
from data_entry_common import flat, rel, traces, unflat

pytestmark = pytest.mark.gpu
KEY = "if_src_update"
MISFIT_TOL, DATA_TOL, YARD, LIVE = 1e-4, 1e-4, 3.0, 1e-2
LAYOUTS = {"one": (1,), "five": (5,), "ragged": (5, 3)}
WIDE = {"w257": (257,), "w513_2": (513, 2)}      # nSteps 65 and 257 only
WIDE_NX = 560
FILTER = [25.0, 60.0, 260.0, 400.0]      # tests/test_gpu_envelope_data.py's
KEYSETS = {"alone": {}, "filter": {"filter": FILTER}, "both": {"filter": FILTER, "if_win": True}}
CASES = [(nt, name) for name in LAYOUTS for nt in DC.NSTEPS] + [(nt, name) for name in WIDE for nt in (65, 257)]
TAPS = (1.3, -0.6)                       # obs[t] = 1.3 syn[t] - 0.6 syn[t - 1]: another source signature


def problem(tmp, nt, layout, keys, name):
    wide = layout in WIDE
    return DC.problem(tmp, nt, (WIDE if wide else LAYOUTS)[layout], KEYSETS[keys], name, misfit_key=KEY, nx=WIDE_NX if wide else 48)


def convolved(syn):
    out = []
    for s in syn:
        o = TAPS[0] * s.astype(np.float64)
        o[:, 1:] += TAPS[1] * s[:, :-1]
        out.append(o)
    return out


def inputs(pb, kind, amp=1.0):
    """-> (obs, syn) with trace amplitude amp: "independent" traces, or obs = the two-tap wavelet on syn + 1e-2 noise"""
    syn = traces(pb, 2, amp)
    if kind == "independent":
        return traces(pb, 1, amp), syn
    return [(o + 1e-2 * n).astype(np.float32) for o, n in zip(convolved(syn), traces(pb, 5, amp))], syn


def reference(O, pb, obs, syn):
    """oracle.conditioned_residual shot by shot -> (misfit, [adjoint source per shot])"""
    total, adj = 0.0, []
    for o, s, sid in zip(obs, syn, G.shots_of(pb)):
        obj, r, _, _ = O.conditioned_residual(o, s, float(pb["para"]["dt"]), O.conditioning_of(pb["para"], pb["survey"], sid))
        total += obj
        adj.append(r)
    return 0.5 * total, adj


# ---- against the oracle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt,layout", CASES)
def test_data_misfit_against_the_oracle(oracle, oracle_nvfma, hip_ops, tmp_path, nt, layout):
    for keys in KEYSETS:
        hip_ops.release()
        pb = problem(tmp_path / keys, nt, layout, keys, "srcupd")
        for kind, amp in [(k, a) for k in ("independent", "wavelet") for a in ((1e-3,) if layout == "one" else (1.0, 1e-3))]:
            obs, syn = inputs(pb, kind, amp)
            f_ref, a_ref = reference(oracle, pb, obs, syn)
            f_alt, a_alt = reference(oracle_nvfma, pb, obs, syn)
            yard = rel(a_alt, a_ref)
            f, a = hip_ops.data_misfit(flat(obs).cuda(), flat(syn).cuda(), pb["Shot_ids"], pb["para_fname"])
            dev = (abs(f - f_ref) / f_ref, rel(unflat(a, obs), a_ref))
            print("source update data nt %d %s %s %s amplitude %g: misfit %.8e (oracle %.8e, relative gap %.2e; its two builds %.2e), adj rel-L2 %.2e (|a| %.4e, two builds %.2e, bound %.2e)"
                  % (nt, layout, keys, kind, amp, f, f_ref, dev[0], abs(f_alt - f_ref) / f_ref, dev[1], G.norm(a_ref), yard, DATA_TOL + YARD * yard))
            assert f_ref > 0 and G.norm(a_ref) > 0 and yard < LIVE, (nt, layout, keys, kind, amp, yard)
            assert dev[0] <= MISFIT_TOL and dev[1] <= DATA_TOL + YARD * yard, (nt, layout, keys, kind, amp, dev, yard)
    hip_ops.release()


# ---- the update absorbs another source signature ---------------------------------------------------------------------------------------------
def test_one_channel_without_noise_is_fitted(oracle, hip_ops, tmp_path):
    """One channel, obs = the two-tap wavelet on syn, no noise: the matching filter IS the wavelet, and the updated misfit is at most 1e-6
    of the plain one (what tests/test_conditioning.py holds the oracle to).  The traces sit under a Gaussian in the middle of the record:
    the update tapers the first samples of the padded gathers, and what it cannot fit there is not what this test is about."""
    hip_ops.release()
    nt = 257
    pb = problem(tmp_path, nt, "one", "alone", "fit")
    t = np.arange(nt) / nt
    syn = [(g * np.exp(-((t - 0.5) / 0.12) ** 2)[None]).astype(np.float32) for g in traces(pb, 2)]
    obs = [o.astype(np.float32) for o in convolved(syn)]
    plain = float(((obs[0].astype(np.float64) - syn[0])[:, 1:] ** 2).sum()) * 0.5
    f, a = hip_ops.data_misfit(flat(obs).cuda(), flat(syn).cuda(), pb["Shot_ids"], pb["para_fname"])
    f_ref, _ = reference(oracle, pb, obs, syn)
    print("source update data fit: updated misfit %.4e (oracle %.4e), plain %.4e, ratio %.2e" % (f, f_ref, plain, f / plain))
    assert plain > 0 and 0 <= f <= 1e-6 * plain and f_ref <= 1e-6 * plain
    hip_ops.release()


# ---- no state from one shot or call to the next ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", ["alone", "both"])
def test_pointers_a_second_call_and_a_single_shot_give_the_same_bits(hip_ops, tmp_path, keys):
    """Host and device pointers and a second call give the same bits; a call on shot 1 alone of the ragged survey (three channels after
    shot 0's five) gives the bits of shot 1 inside the full call, before and after another full call: the matching filter is computed
    from the call's own gathers, nothing of coef_ outlives a shot.  data_gn stays refused."""
    from sepfwi import _native
    hip_ops.release()
    pb = problem(tmp_path, 257, "ragged", keys, "bits")
    obs_l, syn_l = inputs(pb, "wavelet")
    obs, syn = flat(obs_l), flat(syn_l)
    keep = [t.clone() for t in (obs, syn)]
    one = torch.tensor([1], dtype=torch.int32)
    o1, s1 = flat(obs_l[1:]), flat(syn_l[1:])
    f1, a1 = hip_ops.data_misfit(o1.cuda(), s1.cuda(), one, pb["para_fname"])          # the session's first call: shot 1 alone
    fd, ad = hip_ops.data_misfit(obs.cuda(), syn.cuda(), pb["Shot_ids"], pb["para_fname"])
    fh, ah = hip_ops.data_misfit(obs, syn, pb["Shot_ids"], pb["para_fname"])
    f2, a2 = hip_ops.data_misfit(obs.cuda(), syn.cuda(), pb["Shot_ids"], pb["para_fname"])
    f3, a3 = hip_ops.data_misfit(o1.cuda(), s1.cuda(), one, pb["para_fname"])          # ... and after shot 0 has left its filter behind
    assert ad.is_cuda and not ah.is_cuda and ad.abs().max() > 0 and fd > 0
    assert fd == fh == f2 and torch.equal(ad.cpu(), ah) and torch.equal(ad, a2)
    n1 = o1.numel()
    assert a1.abs().max() > 0 and torch.equal(a1, ad[-n1:]) and torch.equal(a3, ad[-n1:]) and f1 == f3 and 0 < f1 < fd
    assert all(torch.equal(a, b) for a, b in zip(keep, (obs, syn))), "an input was changed"
    with pytest.raises(_native.SepFwiError) as e:
        hip_ops.data_gn(syn.cuda(), obs.cuda(), pb["Shot_ids"], pb["para_fname"])
    assert e.value.code == -1 and KEY in str(e.value)
    hip_ops.release()
