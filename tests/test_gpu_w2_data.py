"""The W2 misfit's kernel alone, on the GPU (-m gpu), with no time loop: sepfwi_data_misfit through fwi_ops.data_misfit under if_w2_misfit
on seeded random band-limited traces, against tests/w2_ref.py (float64 on float32 inputs; tests/test_w2_reference.py licenses it).

Shapes: the nSteps of tests/data_entry_common.py and 66, 258, 513, 1025 -- the mass samples nSteps - 1 on both sides of a wave (64) and of
a tile (256) of the block scans, and a second and a fourth tile's carry; one channel, five channels, and two shots with 5 and 3.  Key sets:
the key alone (C: the end taper), with filter, with if_win (channel 1 has weight 0: a dead trace; the last channel of a shot with three or
more an empty window, "Window error 1": its trace passes untouched), with both.  No element and no trace is exempted.

The map is ill-conditioned in its inputs (a relative 3e-5, the distance between a float32 and a float64 band-pass, moves the adjoint source
by up to 6e-3), so the kernel is bounded on IDENTICAL float32 inputs: the reference is fed the library's own fwi_ops.condition output of
obs and syn, and its adjoint source, rounded to float32, goes through the library's own C^T.  Both stages are shipped and held by their
own tests.  The bounds follow from "double arithmetic, rounded once" (EPS = 2^-24, the relative rounding error of float32):
    misfit       |f - f_ref| <= 8 EPS f_ref                     (one rounding of the float32 result)
    window sets  per trace max |a - a_ref| <= 8 EPS max |a_ref|  (C^T pointwise: a one-place flip of the rounded source, carried through)
    filter sets  |a - a_ref| <= 16 EPS |a_ref|                   (C^T linear with norm <= 1, applied alike to both sides)
Against the oracle's own C (a float64 band-pass) the comparison is the suite's: misfit and adjoint source to 1e-4 on the window sets, under
filter to 1e-4 + 3 x the distance of the reference evaluated with the oracle's two transform builds.  Every comparison prints its
deviation before it asserts; profiles/r28_w2_misfit.txt holds the figures measured on the MI355X.

On the parent commit every test fails: the key is unknown there and the file's misfit is L2."""
import numpy as np
import pytest
import torch

import cond_gn_ref as G
import data_entry_common as DC
import w2_ref as W
from data_entry_common import flat, rel, traces
from w2_held import EPS, call, on_identical_inputs

pytestmark = pytest.mark.gpu
ORACLE_TOL, YARD = 1e-4, 3.0
NSTEPS = tuple(sorted(set(DC.NSTEPS) | {66, 258, 513, 1025}))
LAYOUTS = {"one": (1,), "five": (5,), "ragged": (5, 3)}
FILTER = [25.0, 60.0, 260.0, 400.0]      # tests/test_gpu_envelope_data.py's: the lower ramp cuts into the traces' 25 ... 175 Hz
KEYSETS = {"alone": {}, "filter": {"filter": FILTER}, "window": {"if_win": True}, "both": {"filter": FILTER, "if_win": True}}


def problem(tmp, nt, layout, keys, name, **more):
    nrec = LAYOUTS[layout] if isinstance(layout, str) else layout
    return DC.problem(tmp, nt, nrec, dict(KEYSETS[keys], **more), name, misfit_key=W.KEY)


# ---- against the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("nt", NSTEPS)
def test_data_misfit_against_the_reference(oracle, oracle_nvfma, hip_ops, tmp_path, nt, layout):
    for keys in KEYSETS:
        hip_ops.release()
        pb = problem(tmp_path / keys, nt, layout, keys, "w2")
        obs, syn = traces(pb, 1), traces(pb, 2)
        what = "nt %d %s %s" % (nt, layout, keys)
        f, a, f_id, a_id = on_identical_inputs(oracle, hip_ops, pb, obs, syn, what)
        assert nt == 2 or (f_id > 0 and G.norm(a_id) > 0), what      # (one mass sample: both densities are that sample, W = 0)
        # the oracle's own C: float64 transforms, and under filter the distance of its two transform builds as the yardstick
        f_ref, a_ref, _ = W.data_misfit(oracle, pb, obs, syn)
        yard_f = yard_a = 0.0
        if "filter" in KEYSETS[keys]:
            f_alt, a_alt, _ = W.data_misfit(oracle_nvfma, pb, obs, syn)
            yard_f, yard_a = (abs(f_alt - f_ref) / f_ref, rel(a_alt, a_ref)) if f_ref > 0 else (abs(f_alt), G.norm(a_alt))
        dev = (abs(f - f_ref) / f_ref, rel(a, a_ref)) if f_ref > 0 else (abs(f), G.norm(a))
        print("w2 data %s against the oracle's C: misfit gap %.2e (two builds %.2e), adj rel-L2 %.2e (two builds %.2e)" % (what, dev[0], yard_f, dev[1], yard_a))
        assert dev[0] <= ORACLE_TOL + YARD * yard_f and dev[1] <= ORACLE_TOL + YARD * yard_a, (what, dev, yard_f, yard_a)
    hip_ops.release()


@pytest.mark.parametrize("keys", ["alone", "both"])
@pytest.mark.parametrize("nt", [257, 1025])
def test_nearly_fitting_data_meet_the_same_bounds(oracle, hip_ops, tmp_path, nt, keys):
    """syn = obs + 1e-4 noise: W is 1e-8 of an independent pair's, and the bounds are relative to it"""
    hip_ops.release()
    pb = problem(tmp_path, nt, "ragged", keys, "near")
    obs, noise = traces(pb, 1), traces(pb, 2)
    syn = [(o + np.float32(1e-4) * n).astype(np.float32) for o, n in zip(obs, noise)]
    f, a, f_ref, a_ref = on_identical_inputs(oracle, hip_ops, pb, obs, syn, "nearly fitting nt %d %s" % (nt, keys))
    f_ind, _ = call(hip_ops, pb, obs, noise)
    print("w2 data nearly fitting nt %d %s: misfit %.4e, of the independent pair %.4e" % (nt, keys, f, f_ind))
    assert 0 < f < 1e-4 * f_ind
    hip_ops.release()


@pytest.mark.parametrize("keys", list(KEYSETS))
def test_fitting_data_give_nothing(hip_ops, tmp_path, keys):
    """obs = syn: misfit and |a| below 1e-10 of those of the independent pair"""
    hip_ops.release()
    pb = problem(tmp_path, 257, "ragged", keys, "fit")
    obs, syn = traces(pb, 1), traces(pb, 2)
    f0, a0 = call(hip_ops, pb, obs, [o.copy() for o in obs])
    f1, a1 = call(hip_ops, pb, obs, syn)
    print("w2 data obs = syn %s: misfit %.3e and |a| %.3e; independent pair %.3e and %.3e" % (keys, f0, G.norm(a0), f1, G.norm(a1)))
    assert f1 > 0 and G.norm(a1) > 0 and 0 <= f0 <= 1e-10 * f1 and G.norm(a0) <= 1e-10 * G.norm(a1)
    hip_ops.release()


# ---- pointers, repeatability, shot lists ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", ["alone", "both"])
def test_host_and_device_pointers_and_a_second_call_give_the_same_bits(hip_ops, tmp_path, keys):
    hip_ops.release()
    pb = problem(tmp_path, 1025, "ragged", keys, "bits")
    obs, syn = (flat(traces(pb, k)) for k in (1, 2))
    keep = [t.clone() for t in (obs, syn)]
    fd, ad = hip_ops.data_misfit(obs.cuda(), syn.cuda(), pb["Shot_ids"], pb["para_fname"])
    fh, ah = hip_ops.data_misfit(obs, syn, pb["Shot_ids"], pb["para_fname"])
    f2, a2 = hip_ops.data_misfit(obs.cuda(), syn.cuda(), pb["Shot_ids"], pb["para_fname"])
    assert ad.is_cuda and not ah.is_cuda and ad.abs().max() > 0
    assert fd == fh == f2 and torch.equal(ad.cpu(), ah) and torch.equal(ad, a2)
    assert all(torch.equal(a, b) for a, b in zip(keep, (obs, syn))), "an input was changed"
    hip_ops.release()


@pytest.mark.parametrize("keys", ["alone", "both"])
def test_a_single_shot_of_a_ragged_survey_has_the_bits_of_the_full_call(hip_ops, tmp_path, keys):
    hip_ops.release()
    pb = problem(tmp_path, 258, "ragged", keys, "single")
    obs, syn = traces(pb, 1), traces(pb, 2)
    f, a = call(hip_ops, pb, obs, syn)
    parts = []
    for k in range(2):
        fk, ak = call(hip_ops, pb, obs[k:k + 1], syn[k:k + 1], ids=np.asarray([k], np.int32))
        assert fk > 0 and np.array_equal(ak[0], a[k]), (keys, k)
        parts.append(fk)
    print("w2 data single shots %s: %.8e + %.8e, full call %.8e" % (keys, parts[0], parts[1], f))
    assert abs(parts[0] + parts[1] - f) <= 4 * EPS * f      # three float32 roundings of sums formed in double
    hip_ops.release()


@pytest.mark.parametrize("keys", ["alone", "both"])
def test_a_common_power_of_two_changes_no_bit(hip_ops, tmp_path, keys):
    """obs and syn times 2^-10: the same misfit bit for bit (the densities are scaled by the observed trace's peak), a times 2^10 bit for bit"""
    hip_ops.release()
    pb = problem(tmp_path, 513, "ragged", keys, "scale")
    obs, syn = traces(pb, 1), traces(pb, 2)
    s = np.float32(2.0 ** -10)
    f1, a1 = call(hip_ops, pb, obs, syn)
    f2, a2 = call(hip_ops, pb, [o * s for o in obs], [y * s for y in syn])
    assert f1 > 0 and f1 == f2 and all(np.array_equal(x * np.float32(2.0 ** 10), y) for x, y in zip(a1, a2))
    hip_ops.release()


# ---- what the misfit is for -----------------------------------------------------------------------------------------------------------------
def test_misfit_grows_with_the_shift_over_one_and_a_half_periods(hip_ops, tmp_path):
    """three two-arrival 15 Hz Ricker traces (one channel per shot, so that every trace has a misfit of its own), the synthetic one
    shifted by 0 ... 100 ms: strictly increasing, where the L2 misfit of the same traces turns back"""
    hip_ops.release()
    pb = problem(tmp_path, 600, (1, 1, 1), "alone", "shift")
    arrivals = [(0.20, 0.32), (0.15, 0.30), (0.25, 0.36)]
    shifts = [0.01 * k for k in range(11)]
    for k, t0 in enumerate(arrivals):
        o = W.ricker_pair(600, DC.DT, 15.0, t0).astype(np.float32)[None, :]
        vals, l2 = [], []
        for sh in shifts:
            s = W.ricker_pair(600, DC.DT, 15.0, t0, shift=sh).astype(np.float32)[None, :]
            vals.append(call(hip_ops, pb, [o], [s], ids=np.asarray([k], np.int32))[0])
            l2.append(float(((o.astype(np.float64) - s) ** 2).sum()))
        print("w2 data shifts, trace %d: W2 %s; L2 %s" % (k, " ".join("%.3e" % v for v in vals), " ".join("%.3e" % v for v in l2)))
        assert all(b > a for a, b in zip(vals, vals[1:])), (k, vals)
        assert not all(b > a for a, b in zip(l2, l2[1:])), (k, l2)
    hip_ops.release()


def test_data_gn_is_refused(hip_ops, tmp_path):
    from sepfwi import _native
    hip_ops.release()
    pb = problem(tmp_path, 64, "five", "both", "gn")
    x = flat(traces(pb, 1)).cuda()
    with pytest.raises(_native.SepFwiError) as e:
        hip_ops.data_gn(x, x, pb["Shot_ids"], pb["para_fname"])
    assert e.value.code == -1 and "if_w2_misfit" in str(e.value)
    hip_ops.release()
