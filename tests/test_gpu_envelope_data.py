"""The envelope misfit's kernels alone, on the GPU (-m gpu), with no time loop: sepfwi_data_misfit and sepfwi_data_gn through
fwi_ops.data_misfit / data_gn on seeded random band-limited traces, against tests/envelope_ref.py (float64 on float32 inputs; C and C^T the
oracle's, tests/test_envelope_reference.py licenses it).

Shapes: a 40 x 48 grid with 10-cell layers (only the channel counts matter), nSteps 2, 3 (the shortest transforms), 63, 64, 65 (a
wavefront of the per-trace reduction), 255, 256, 257 (its block) and 600; one channel, five channels, and two shots with 5 and 3 channels
(an FFT plan per trace count).  Key sets: the key alone (C: the end taper), with filter, with if_win (channel 1 has weight 0, the last
channel of a shot with three or more an empty window: "Window error 1", its trace passes untouched), with both.

Tolerances, none new: the misfit to the suite's 1e-4; adj and out to rel-L2 1e-4, the seismogram tolerance that C itself is held to in
tests/test_gpu_conditioned_gauss_newton.py; the symmetry of data_gn to 1e-3 of sqrt(<d, G d> <u, G u>), the bound of the exact adjoint's
symmetry checks (tests/exact_adjoint_ref.py: held).  Every comparison prints its deviation before it asserts;
profiles/r21_envelope_misfit.txt holds the figures measured on the MI355X.

On the parent commit every test fails: fwi_ops has no data_misfit / data_gn."""
import numpy as np
import pytest
import torch

import cond_gn_ref as G
import data_entry_common as DC
import envelope_ref as E
from data_entry_common import flat, rel, traces, unflat

pytestmark = pytest.mark.gpu
MISFIT_TOL, DATA_TOL, SYM_TOL = 1e-4, 1e-4, 1e-3
NSTEPS = DC.NSTEPS
LAYOUTS = {"one": (1,), "five": (5,), "ragged": (5, 3)}
FILTER = [25.0, 60.0, 260.0, 400.0]      # the traces carry 25 ... 175 Hz: the lower ramp cuts into them; the one live bin of nSteps = 2 (250 Hz) passes
KEYSETS = {"alone": {}, "filter": {"filter": FILTER}, "window": {"if_win": True}, "both": {"filter": FILTER, "if_win": True}}


def problem(tmp, nt, layout, keys, name, misfit_key=E.KEY):
    """data_entry_common.problem with the channel counts of LAYOUTS[layout]"""
    return DC.problem(tmp, nt, LAYOUTS[layout], keys, name, misfit_key)


# ---- against the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("nt", NSTEPS)
def test_data_misfit_and_data_gn_against_the_reference(oracle, hip_ops, tmp_path, nt, layout):
    for keys in KEYSETS:
        hip_ops.release()
        pb = problem(tmp_path / keys, nt, layout, KEYSETS[keys], "env")
        obs, syn, d = traces(pb, 1), traces(pb, 2), traces(pb, 3)
        f_ref, a_ref, _, _ = E.data_misfit(oracle, pb, obs, syn)
        g_ref = E.data_gn(oracle, pb, syn, d)
        f, a = hip_ops.data_misfit(flat(obs).cuda(), flat(syn).cuda(), pb["Shot_ids"], pb["para_fname"])
        g = hip_ops.data_gn(flat(syn).cuda(), flat(d).cuda(), pb["Shot_ids"], pb["para_fname"])
        dev = (abs(f - f_ref) / f_ref, rel(unflat(a, obs), a_ref), rel(unflat(g, obs), g_ref))
        print("envelope data nt %d %s %s: misfit %.8e (reference %.8e, relative gap %.2e), adj rel-L2 %.2e, data_gn rel-L2 %.2e" % (nt, layout, keys, f, f_ref, *dev))
        assert f_ref > 0 and G.norm(a_ref) > 0 and G.norm(g_ref) > 0
        assert dev[0] <= MISFIT_TOL and dev[1] <= DATA_TOL and dev[2] <= DATA_TOL, (nt, layout, keys, dev)
    hip_ops.release()


# ---- pointers and repeatability -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", ["alone", "both"])
def test_host_and_device_pointers_and_a_second_call_give_the_same_bits(hip_ops, tmp_path, keys):
    hip_ops.release()
    pb = problem(tmp_path, 257, "ragged", KEYSETS[keys], "bits")
    obs, syn, d = (flat(traces(pb, k)) for k in (1, 2, 3))
    keep = [t.clone() for t in (obs, syn, d)]
    fd, ad = hip_ops.data_misfit(obs.cuda(), syn.cuda(), pb["Shot_ids"], pb["para_fname"])
    fh, ah = hip_ops.data_misfit(obs, syn, pb["Shot_ids"], pb["para_fname"])
    f2, a2 = hip_ops.data_misfit(obs.cuda(), syn.cuda(), pb["Shot_ids"], pb["para_fname"])
    assert ad.is_cuda and not ah.is_cuda and ad.abs().max() > 0
    assert fd == fh == f2 and torch.equal(ad.cpu(), ah) and torch.equal(ad, a2)
    gd = hip_ops.data_gn(syn.cuda(), d.cuda(), pb["Shot_ids"], pb["para_fname"])
    gh = hip_ops.data_gn(syn, d, pb["Shot_ids"], pb["para_fname"])
    g2 = hip_ops.data_gn(syn.cuda(), d.cuda(), pb["Shot_ids"], pb["para_fname"])
    assert gd.is_cuda and not gh.is_cuda and gd.abs().max() > 0 and torch.equal(gd.cpu(), gh) and torch.equal(gd, g2)
    assert all(torch.equal(a, b) for a, b in zip(keep, (obs, syn, d))), "an input was changed"
    with pytest.raises(ValueError, match="elements"):
        hip_ops.data_misfit(obs[:-1], syn[:-1], pb["Shot_ids"], pb["para_fname"])
    hip_ops.release()


# ---- symmetry and sign -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", list(KEYSETS))
def test_data_gn_is_symmetric_and_non_negative(hip_ops, tmp_path, keys):
    hip_ops.release()
    pb = problem(tmp_path, 257, "ragged", KEYSETS[keys], "sym")
    syn, d, u = traces(pb, 2), traces(pb, 3), traces(pb, 4)
    gd = unflat(hip_ops.data_gn(flat(syn).cuda(), flat(d).cuda(), pb["Shot_ids"], pb["para_fname"]), d)
    gu = unflat(hip_ops.data_gn(flat(syn).cuda(), flat(u).cuda(), pb["Shot_ids"], pb["para_fname"]), d)
    dd, uu, ud, du = G.dot(d, gd), G.dot(u, gu), G.dot(u, gd), G.dot(d, gu)
    scale = float(np.sqrt(dd * uu))
    print("envelope data symmetry %s: <d, G d> %.8e, <u, G u> %.8e, <u, G d> %.8e, <d, G u> %.8e, gap %.2e of sqrt(<d, G d> <u, G u>)" % (keys, dd, uu, ud, du, abs(ud - du) / scale))
    assert dd > 0 and uu > 0 and abs(ud - du) <= SYM_TOL * scale
    hip_ops.release()


# ---- the existing misfits through the new entry point -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("misfit", ["l2", "l2_plain", "cross"])
def test_existing_misfits_through_data_misfit(oracle, hip_ops, tmp_path, misfit):
    """An L2 file (with window and filter; and with no conditioning key at all) and an if_cross_misfit file: data_misfit reproduces
    oracle.conditioned_residual to the same tolerances; data_gn is C^T Z C d under L2 and refused (-1) under if_cross_misfit."""
    hip_ops.release()
    keys = {} if misfit == "l2_plain" else KEYSETS["both"]
    pb = problem(tmp_path, 257, "ragged", keys, misfit, misfit_key="if_cross_misfit" if misfit == "cross" else None)
    obs, syn, d = traces(pb, 1), traces(pb, 2), traces(pb, 3)
    dt, total, a_ref, g_ref = float(pb["para"]["dt"]), 0.0, [], []
    for o, s, x, sid in zip(obs, syn, d, G.shots_of(pb)):
        cond = oracle.conditioning_of(pb["para"], pb["survey"], sid)
        if cond is None:      # no key: C = 1
            r = E.Z(o.astype(np.float64) - s)
            total += float((r * r).sum())
            a_ref.append(r.astype(np.float32))
            g_ref.append(E.Z(x).astype(np.float32))
            continue
        obj, r, _, _ = oracle.conditioned_residual(o, s, dt, cond)
        total += obj
        a_ref.append(r)
        g_ref.append(G.Ct_of(oracle, pb, G.Z(G.C_of(oracle, pb, x, sid)), sid))
    f_ref = 0.5 * total
    f, a = hip_ops.data_misfit(flat(obs).cuda(), flat(syn).cuda(), pb["Shot_ids"], pb["para_fname"])
    dev = (abs(f - f_ref) / abs(f_ref), rel(unflat(a, obs), a_ref))
    print("envelope data %s file: misfit %.8e (oracle %.8e, relative gap %.2e), adj rel-L2 %.2e" % (misfit, f, f_ref, *dev))
    assert dev[0] <= MISFIT_TOL and dev[1] <= DATA_TOL
    if misfit == "cross":
        from sepfwi import _native
        with pytest.raises(_native.SepFwiError) as e:
            hip_ops.data_gn(flat(syn).cuda(), flat(d).cuda(), pb["Shot_ids"], pb["para_fname"])
        assert e.value.code == -1 and "if_cross_misfit" in str(e.value)
    else:
        g = hip_ops.data_gn(flat(syn).cuda(), flat(d).cuda(), pb["Shot_ids"], pb["para_fname"])
        print("envelope data %s file: data_gn rel-L2 %.2e" % (misfit, rel(unflat(g, obs), g_ref)))
        assert rel(unflat(g, obs), g_ref) <= DATA_TOL
    hip_ops.release()


def test_data_entry_points_refuse_if_src_update(oracle, hip_ops, tmp_path):
    """data_gn is refused (-1) under if_src_update; data_misfit is served: the misfit and adjoint source of
    oracle.conditioned_residual(..., src_update=True) to the same tolerances (tests/test_gpu_source_update_data.py holds it at every
    shape)."""
    from sepfwi import _native
    hip_ops.release()
    pb = problem(tmp_path, 64, "five", {}, "srcupd", misfit_key="if_src_update")
    obs, syn = traces(pb, 1), traces(pb, 2)
    x = flat(obs).cuda()
    with pytest.raises(_native.SepFwiError) as e:
        hip_ops.data_gn(x, x, pb["Shot_ids"], pb["para_fname"])
    assert e.value.code == -1 and "if_src_update" in str(e.value)
    obj, a_ref, _, _ = oracle.conditioned_residual(obs[0], syn[0], float(pb["para"]["dt"]), oracle.conditioning_of(pb["para"], pb["survey"], 0))
    f, a = hip_ops.data_misfit(x, flat(syn).cuda(), pb["Shot_ids"], pb["para_fname"])
    dev = (abs(f - 0.5 * obj) / (0.5 * obj), rel(unflat(a, obs), [a_ref]))
    print("envelope data if_src_update file: misfit %.8e (oracle %.8e, relative gap %.2e), adj rel-L2 %.2e" % (f, 0.5 * obj, *dev))
    assert obj > 0 and G.norm([a_ref]) > 0 and dev[0] <= MISFIT_TOL and dev[1] <= DATA_TOL
    hip_ops.release()
