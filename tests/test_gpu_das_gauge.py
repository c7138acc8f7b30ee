"""DAS gauge length (parameter key "das_gauge_length", csrc/das_gauge.{hpp,cpp,hip}) on the GPU: each channel records the mean axial
strain over G cells along the fibre, and its adjoint source is the exact transpose.

The oracle knows one-cell channels only, so it is always given the EXPANDED member survey -- one channel at p + k a per member k of
every gauge, same sensitivities -- and the gauge is formed from its gathers with the weights w_k (never a file with the key)."""
import json
import os

import numpy as np
import pytest
import torch

import problems as P
import gauge_ref as R
from fuzz_common import write_para
from gauge_ref import gauge_of, member_survey, members
from sepfwi import _native
from sepfwi import utils as ft

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-3
CASES = {"horizontal-3": ("horizontal", 3), "horizontal-4": ("horizontal", 4), "vertical-3": ("vertical", 3), "directional-2": ("directional", 2)}


def gauge_problem(tmp_path, fiber, G, nshots=2, **kw):
    opts = dict(nz=300, nx=500, nPml=10, nSteps=420, nshots=nshots, hetero=True, rec_z=40)
    if fiber == "vertical":
        opts.update(das_fiber="vertical", src_x=[200, 330][:nshots])
    elif fiber == "directional":
        opts.update(das_sensitivity="random", nrec_stride=2)
    opts.update(kw)
    pb = P.make_problem(str(tmp_path), **opts)
    d = pb["para"]["dz"] if fiber == "vertical" else pb["para"]["dx"]
    fn, para = write_para(pb, "gauge", das_gauge_length=G * d)
    return pb, fn, para


def gathers(data_dir, ids, nS):
    return {c: np.stack([ft.read_shot_gather(data_dir, c, int(i), nS) for i in ids]) for c in ("pr", "vx", "vz", "ett")}


@pytest.mark.parametrize("case", sorted(CASES))
def test_gauge_forward_and_gradient_match_oracle_member_survey(tmp_path, oracle, hip_ops, case):
    """Forward: the gauge gathers equal sum_k w_k x the oracle's ett of the member survey (1e-4 rel-L2), pr / vx / vz are bit-identical
    to the library's run without the key.  Gradient: observed data are the true-model gauge gathers; the oracle runs the member survey
    with obs'_j = syn_init_j + w_j r_c, so that each member's residual is w_j times its channel's -- gLambda / gMu / gDen / gStf to 1e-3,
    the misfit to 1/2 sum r_c^2 formed from the oracle's seismograms to 1e-4."""
    fiber, G = CASES[case]
    pb, fn, para = gauge_problem(tmp_path, fiber, G)
    nS, ids = pb["nSteps"], pb["Shot_ids"]
    vertical = fiber == "vertical"
    msurvey = member_survey(pb["survey"], G, vertical)
    mpara = dict(pb["para"])
    lt, mt, dt_ = pb["lame_true"]
    lam, mu, den = pb["lame_init"]
    lam = (lam * 1.05).contiguous()       # (the models' anomalies lie beyond the channels' reach in these few steps)
    # forward
    hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, ids, fn)
    got = gathers(para["data_dir_name"], ids.tolist(), nS)
    fn_pt, para_pt = write_para(pb, "point")
    hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, ids, fn_pt)
    pt = gathers(para_pt["data_dir_name"], ids.tolist(), nS)
    for c in ("pr", "vx", "vz"):
        assert np.array_equal(got[c], pt[c]), c
    assert not np.array_equal(got["ett"], pt["ett"])
    ref_true = oracle.cufd(lt.numpy(), mt.numpy(), dt_.numpy(), pb["Stf"].numpy(), 2, ids.numpy(), mpara, msurvey)["syn"]
    want = gauge_of(ref_true[:, 3], G)
    fwd = P.rel_l2(got["ett"], want)
    # gradient
    obs = got["ett"]                                               # the library's true-model gauge gathers (the files just written)
    syn_init = oracle.cufd(lam.numpy(), mu.numpy(), den.numpy(), pb["Stf"].numpy(), 2, ids.numpy(), mpara, msurvey)["syn"]
    r = obs.astype(np.float64) - gauge_of(syn_init[:, 3], G)
    r[:, :, 0] = 0.0                                               # first time sample (k_residual)
    _, w = members(G)
    obs_m = syn_init.copy()
    g, n, _ = r.shape
    obs_m[:, 3] = (syn_init[:, 3].reshape(g, n, w.size, nS) + w[None, None, :, None] * r[:, :, None, :]).reshape(g, n * w.size, nS).astype(np.float32)
    ref = oracle.cufd(lam.numpy(), mu.numpy(), den.numpy(), pb["Stf"].numpy(), 1, ids.numpy(), mpara, msurvey, obs=obs_m)
    m, gL, gM, gD, gS = [t.numpy().copy() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, ids, fn)]
    misfit_ref = 0.5 * float(np.sum(r * r))
    dev = {"fwd ett": fwd, "misfit": abs(float(m[0]) - misfit_ref) / misfit_ref}
    for key, a in (("gLambda", gL), ("gMu", gM), ("gDen", gD)):
        dev[key] = (P.rel_l2(a, ref[key]), float(np.abs(a - ref[key]).max() / np.abs(ref[key]).max()))
    dev["gStf"] = P.rel_l2(gS[:len(ids)], ref["gStf"])
    print("gauge %s: %r" % (case, dev))
    assert fwd <= 1e-4, dev
    assert misfit_ref > 0 and dev["misfit"] <= 1e-4, dev
    for key in ("gLambda", "gMu", "gDen"):
        assert np.abs(ref[key]).max() > 0
        assert dev[key][0] <= GRAD_TOL and dev[key][1] <= GRAD_TOL, (key, dev)
    assert dev["gStf"] <= GRAD_TOL, dev


@pytest.mark.parametrize("case", ["horizontal-3", "directional-2"])
def test_gauge_every_schedule_agrees(tmp_path, hip_ops, probes_lib, case):
    """The same gauge channels through every schedule (300 x 500 grid: 2 880 row segments, enough for the persistent loop):
    the loop (batch=0) -- every backward step inside it -- against the two-launch step (batch=0, bwd_fuse=2), the reference's launch
    structure (bwd_fuse=0) and the batched schedule.  Gauge targets are distinct and each gets ONE add of the value folded in entry order
    per step, in the loop (k_inject_values + GINJ) as in k_inject_gauge: bit for bit.  The batched schedule with one backward lane
    (batch_b=1) too; with a lane per shot (the default) the lanes' imaging accumulators are summed at the end -- the same terms in
    another order -- so there the gradients agree to 5e-6 and misfit, source gradient and gathers bit for bit.
    (Whole test on the -DSEPFWI_PROBES build, which alone takes batch_b.)"""
    fiber, G = CASES[case]
    pb, fn, para = gauge_problem(tmp_path, fiber, G, nrec_stride=1)      # horizontal, stride 1: a line -- that the gauge must not fuse
    nS, ids = pb["nSteps"], pb["Shot_ids"]
    lt, mt, dt_ = pb["lame_true"]
    lam, mu, den = pb["lame_init"]
    lam = (lam * 1.05).contiguous()       # (the models' anomalies lie beyond the channels' reach in these few steps)
    fwd = {}
    for name, opts in (("streams", dict(batch=0)), ("batched", dict(batch=1))):
        with P.kernel_options(**opts):
            hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, ids, fn)
            fwd[name] = gathers(para["data_dir_name"], ids.tolist(), nS)
    for c in fwd["streams"]:
        assert np.array_equal(fwd["streams"][c], fwd["batched"][c]), c
    out, steps = {}, {}
    for name, opts in (("loop", dict(batch=0, bwd_fuse=4)), ("two-launch", dict(batch=0, bwd_fuse=2)), ("reference launches", dict(batch=0, bwd_fuse=0)),
                       ("batched", dict(batch=1)), ("batched, one backward lane", dict(batch=1, batch_b=1))):
        with P.kernel_options(**opts):
            out[name] = [t.numpy().copy() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, ids, fn)]
            steps[name] = hip_ops.stats(fn, 0)["persist_steps"]
    assert steps["loop"] == len(ids) * (nS - 1), (steps, hip_ops.loop_status(fn))
    assert all(v == 0 for k, v in steps.items() if k != "loop"), steps
    assert out["loop"][0][0] > 0 and np.abs(out["loop"][1]).max() > 0
    for name in ("loop", "reference launches", "batched, one backward lane"):
        for k, (a, b) in enumerate(zip(out[name], out["two-launch"])):
            assert np.array_equal(a, b), (name, k, float(np.abs(a - b).max()))
    for k in (0, 4):
        assert np.array_equal(out["batched"][k], out["two-launch"][k]), k
    for k in (1, 2, 3):
        assert P.rel_l2(out["batched"][k], out["two-launch"][k]) <= 5e-6, k


def test_gauge_of_one_cell_is_the_plain_channel(tmp_path, hip_ops):
    """das_gauge_length == dx (G = 1): all five outputs bit-identical to a file without the key."""
    pb = P.make_problem(str(tmp_path), nz=300, nx=500, nPml=10, nSteps=300, nshots=2, hetero=True, rec_z=40, nrec_stride=3)
    lt, mt, dt_ = pb["lame_true"]
    lam, mu, den = pb["lame_init"]
    lam = (lam * 1.05).contiguous()       # (the models' anomalies lie beyond the channels' reach in these few steps)
    hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    para = dict(pb["para"], das_gauge_length=pb["para"]["dx"])      # same data directory: the same observed gathers
    fn = os.path.join(str(tmp_path), "one_cell.json")
    with open(fn, "w") as fp:
        json.dump(para, fp)
    a = [t.numpy().copy() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])]
    b = [t.numpy().copy() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, pb["Shot_ids"], fn)]
    assert a[0][0] > 0
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), k


@pytest.mark.parametrize("length,code", [(15.0, -5), (0.0, -5), (-30.0, -5), (310.0, -1)], ids=["non-integer", "zero", "negative", "outside"])
def test_gauge_errors_reach_the_c_abi(tmp_path, hip_ops, length, code):
    """A gauge that is not a whole number of cells or not positive is a parameter-file error (SEPFWI_EJSON, like the other keys); one
    whose members reach outside the grid is refused by the survey check (SEPFWI_EINVAL) and names the shot and the channel."""
    pb = P.make_problem(str(tmp_path), nz=60, nx=80, nPml=10, nSteps=50, nshots=1, hetero=False)
    para = dict(pb["para"], das_gauge_length=length)
    with open(pb["para_fname"], "w") as fp:
        json.dump(para, fp)
    lt, mt, dt_ = pb["lame_true"]
    with pytest.raises(_native.SepFwiError) as e:
        hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    assert e.value.code == code, str(e.value)
    if code == -1:
        assert "receiver 0 of shot 0" in str(e.value), str(e.value)
    assert "das_gauge_length" in str(e.value) or code == -1
    # the library is fine afterwards
    with open(pb["para_fname"], "w") as fp:
        json.dump(pb["para"], fp)
    hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])


@pytest.mark.timeout(600)
def test_gauge_at_headline_size_loop_matches_two_launch(tmp_path, hip_ops):
    """bench.py's 2000 x 1000 model and channel line with G = 3, 300 steps, one shot: the backward pass runs in the persistent loop (strip
    order at this size) and equals the two-launch step bit for bit."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    nS = 300
    pb = bench.setup_problem(str(tmp_path), 1000, 2000, nS, 1)
    with open(pb["para_fname"]) as fp:
        para = json.load(fp)
    para["das_gauge_length"] = 3 * para["dx"]
    with open(pb["para_fname"], "w") as fp:
        json.dump(para, fp)
    nzc, nseg = pb["nz_pad"] - pb["nPad"], (pb["nx_pad"] + 63) // 64
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert nzc * nseg >= 56 * 2 * ncu, (nzc, nseg, ncu)              # strip order (session_persist.cpp tile-size rule)
    ids = torch.tensor([0], dtype=torch.int32)
    lt, mt, dt_ = [t.cuda() for t in pb["lame_true"]]
    lam, mu, den = [t.cuda() for t in pb["lame_init"]]
    hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, ids, pb["para_fname"], to_store=True)
    loop = [t.cpu() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, ids, pb["para_fname"])]
    assert hip_ops.stats(pb["para_fname"], 0)["persist_steps"] == nS - 1, hip_ops.loop_status(pb["para_fname"])
    with P.kernel_options(bwd_fuse=2):
        two = [t.cpu() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, ids, pb["para_fname"])]
        assert hip_ops.stats(pb["para_fname"], 0)["persist_steps"] == 0
    hip_ops.release()
    assert float(loop[0]) > 0 and float(loop[1].abs().max()) > 0
    for k, (a, b) in enumerate(zip(loop, two)):
        assert torch.equal(a, b), (k, float((a - b).abs().max()))


# ---- the crossings the random draws of tests/test_gpu_gauge_fuzz.py cannot reach ----------------------------------------------------
COND_GAUGES = {"horizontal-3": ("horizontal", 3), "vertical-4": ("vertical", 4)}


def _write_observed(data_dir, ids, ett, own):
    os.makedirs(data_dir, exist_ok=True)
    for i, sid in enumerate(ids):
        np.ascontiguousarray(ett[i], dtype=np.float32).tofile(os.path.join(data_dir, "Shot_ett%d.bin" % sid))
        for k, c in enumerate(("pr", "vx", "vz")):
            np.ascontiguousarray(own[i][k]).tofile(os.path.join(data_dir, "Shot_%s%d.bin" % (c, sid)))


@pytest.mark.parametrize("mode", ["filter", "window", "cross", "all", "srcupd", "srcupd_all"])
@pytest.mark.parametrize("gauge", sorted(COND_GAUGES))
@pytest.mark.parametrize("opts", [dict(), dict(batch=0)], ids=["default", "streams"])
def test_gauge_conditioning_matches_oracle(tmp_path, oracle, oracle_nvfma, hip_ops, mode, gauge, opts):
    """The data-conditioning chain on gauge channels: the six modes of test_conditioning.py::test_hip_conditioning_matches_oracle (its
    problem, its keys, its tolerances and its gStf yardstick) with G = 3 on a horizontal and G = 4 on a vertical fibre, against
    gauge_ref.reference -- windows, band-pass, cross-correlation misfit and source update act on the GAUGE gathers, and member j of
    channel c is handed w_j times the conditioned adjoint source of c."""
    fiber, G = COND_GAUGES[gauge]
    pb = P.cond_problem(tmp_path, mode, **(dict(das_fiber="vertical") if fiber == "vertical" else {}))
    para, sv = pb["para"], pb["survey"]
    para["das_gauge_length"] = G * (para["dz"] if fiber == "vertical" else para["dx"])
    json.dump(para, open(pb["para_fname"], "w"))
    ids = pb["Shot_ids"].numpy()
    stf = pb["Stf"].numpy()
    stf_obs = stf
    if mode.startswith("srcupd"):   # the observations come from ANOTHER source signature: delayed, scaled, with a second lobe
        stf_obs = 1.6 * np.roll(stf, 4, axis=1) - 0.5 * np.roll(stf, 11, axis=1)
        stf_obs[:, :11] = 0.0
    gauge_t, own_t = R.forward(oracle, [t.numpy() for t in pb["lame_true"]], stf_obs, ids, para, sv, G)
    obs = [a.astype(np.float32) for a in gauge_t]
    _write_observed(pb["data_dir"], ids.tolist(), obs, own_t)
    init = [t.numpy() for t in pb["lame_init"]]
    ref = R.reference(oracle, init, stf, ids, para, sv, G, obs)
    ref_plain = R.reference(oracle, init, stf, ids, {k: v for k, v in para.items() if k not in R.COND_KEYS}, sv, G, obs)
    assert P.rel_l2(ref["gMu"], ref_plain["gMu"]) > 0.05          # the conditioning does change the problem
    lam, mu, den = pb["lame_init"]
    with P.kernel_options(**opts):
        m, gL, gM, gD, gS = hip_ops.backward(lam, mu, den, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
        l2 = lambda a: float(np.linalg.norm(np.asarray(a, np.float64)))
        nS_ = ref["gStf"].shape[0]
        dev = {"misfit": abs(float(m) - ref["misfit"]) / abs(ref["misfit"]), "gStf": l2(gS.numpy()[:nS_] - ref["gStf"]) / l2(ref["gStf"])}
        for key, g in (("gLambda", gL), ("gMu", gM), ("gDen", gD)):
            dev[key] = P.rel_l2(g.numpy(), ref[key])
        print("gauge conditioning %s %s %r: %r" % (gauge, mode, opts, dev))
        assert dev["misfit"] <= 1e-4, dev
        for key in ("gLambda", "gMu", "gDen"):
            assert dev[key] <= 1e-3, (key, dev)
        # the source gradient of the cross-correlation misfit is a cancellation residue: the yardstick of test_hip_conditioning_matches_oracle
        two_roundings = 0.0
        if mode in ("cross", "all"):
            alt = R.reference(oracle_nvfma, init, stf, ids, para, sv, G, obs)
            two_roundings = 3.0 * l2(alt["gStf"] - ref["gStf"])
        assert l2(gS.numpy()[:nS_] - ref["gStf"]) <= 1e-3 * l2(ref["gStf"]) + two_roundings, (mode, dev)
        m0 = hip_ops.forward(lam, mu, den, pb["Stf"], 0, pb["Shot_ids"], pb["para_fname"])[0]     # misfit-only entry point
        assert abs(float(m0) - float(m)) <= 1e-6 * abs(float(m))


def test_gauge_observed_data_routes_agree(tmp_path, hip_ops, probes_lib):
    """One gauge problem (G = 4, four shots, gathers of 0.48 MB) with the observed gathers from the Shot_*.bin files, handed over by
    set_observed, observed into the store (to_store=True), from a packed file, and with a store budget of 1 MB -- two gathers -- that
    spills to pinned host memory: misfit, the three gradients and the source gradient bit for bit in all five (the patterns of
    test_observed_data_from_memory_equals_files, test_observe_into_the_store_equals_the_file_route,
    test_packed_observed_file_equals_the_per_shot_files and test_bounded_observed_store_spills_to_pinned_host)."""
    nshots = 4
    pb = P.make_problem(str(tmp_path), nz=40, nx=130, nPml=10, nSteps=1000, nshots=nshots, hetero=True)
    gather = pb["nrec"] * pb["nSteps"] * 4
    assert 2 * gather <= 1000000 < 3 * gather
    fn, para = write_para(pb, "gauge", das_gauge_length=4 * pb["para"]["dx"])
    ids, nS = pb["Shot_ids"], pb["nSteps"]
    lt, mt, dt_ = pb["lame_true"]
    lam, mu, den = pb["lame_init"]
    lam = (lam * 1.05).contiguous()
    run = lambda f: [t.numpy().copy() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, ids, f)]
    with P.kernel_options(batch=0, fwd_lanes=2):
        hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, ids, fn)
        ett = [ft.read_shot_gather(para["data_dir_name"], "ett", int(i), nS) for i in ids]
        ref = run(fn)
        assert ref[0][0] > 0 and np.abs(ref[1]).max() > 0 and np.abs(ref[4]).max() > 0
        # a packed file instead of the per-shot files
        pack = os.path.join(str(tmp_path), "gauge_ett.pack")
        ft.pack_observed(para["data_dir_name"], ids.tolist(), nS, pack)
        hip_ops.release()
        for f in os.listdir(para["data_dir_name"]):
            os.remove(os.path.join(para["data_dir_name"], f))
        fn_pack = os.path.join(str(tmp_path), "gauge_packed.json")
        json.dump(dict(para, obs_pack_fname=pack), open(fn_pack, "w"))
        out = {"packed file": run(fn_pack)}
        # handed over from memory (device and host pointers), no file anywhere
        hip_ops.release()
        for i, sid in enumerate(ids.tolist()):
            t = torch.tensor(ett[i])
            hip_ops.set_observed(fn, sid, t.cuda() if i % 2 else t)
        out["set_observed"] = run(fn)
        # observed into the store
        hip_ops.release()
        hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, ids, fn, to_store=True)
        assert os.listdir(para["data_dir_name"]) == []
        out["to_store"] = run(fn)
        st = hip_ops.stats(fn, 0)
        assert st["obs_device_bytes"] == nshots * gather and st["obs_evictions"] == 0, st
    hip_ops.release()
    with P.kernel_options(batch=0, fwd_lanes=2, obs_cache_mb=1):
        hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, ids, fn, to_store=True)      # the budget in force: the store spills while it is filled
        out["store of 1 MB"] = run(fn)
        st = hip_ops.stats(fn, 0)
        assert 0 < st["obs_device_bytes"] <= 1000000 and st["obs_host_bytes"] >= (nshots - 2) * gather and st["obs_evictions"] >= nshots - 2, st
    for name, got in out.items():
        for k, (a, b) in enumerate(zip(got, ref)):
            assert np.array_equal(a, b), (name, k, float(np.abs(a - b).max()))


@pytest.mark.parametrize("opts", [dict(), dict(batch=0), dict(batch=0, bwd_fuse=2)], ids=["default", "streams", "two-launch"])
def test_quiet_skip_stays_off_for_gauge_channels(tmp_path, hip_ops, opts):
    """Option quiet_skip with gauge channels: they are not sampled at their own cells, so the quiet maps are not taken for them
    (the `!gauge` of Session::make_ctx's line test) -- gathers, misfit and gradients bit-identical to quiet_skip=0, and
    stats()["quiet_total"] == 0: no map was in use.  (An adjoint source added to a segment marked quiet would be a silent gradient
    error.)  The channels are a line of CONSECUTIVE cells inside the computed region, the one receiver geometry the option is taken
    for: the same problem without the key -- the positive control at the end -- does run with the maps (quiet_total > 0)."""
    pb, fn, para = gauge_problem(tmp_path, "horizontal", 3, nrec_stride=1)
    nS, ids = pb["nSteps"], pb["Shot_ids"]
    lt, mt, dt_ = pb["lame_true"]
    lam, mu, den = pb["lame_init"]
    lam = (lam * 1.05).contiguous()
    res = {}
    for q in (0, 1):
        with P.kernel_options(quiet_skip=q, **opts):
            hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, ids, fn)
            data = gathers(para["data_dir_name"], ids.tolist(), nS)
            out = [t.numpy().copy() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, ids, fn)]
            res[q] = (data, out, hip_ops.stats(fn, 0))
        hip_ops.release()
    assert res[0][1][0][0] > 0 and np.abs(res[0][1][1]).max() > 0 and np.abs(res[0][1][4]).max() > 0
    for c in res[0][0]:
        assert np.array_equal(res[0][0][c], res[1][0][c]), c
    for k, (a, b) in enumerate(zip(res[0][1], res[1][1])):
        assert np.array_equal(a, b), (opts, k, float(np.abs(a - b).max()))
    assert res[0][2]["quiet_total"] == 0 and res[1][2]["quiet_total"] == 0, (res[0][2], res[1][2])
    # positive control: the same channels without the key are a fused line, and the option is taken for it
    with P.kernel_options(quiet_skip=1, **opts):
        hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, ids, pb["para_fname"])
        hip_ops.backward(lam, mu, den, pb["Stf"], 1, ids, pb["para_fname"])
        st = hip_ops.stats(pb["para_fname"], 0)
    hip_ops.release()
    assert st["quiet_total"] > 0 and 0 < st["quiet_active"] <= st["quiet_total"], (opts, st)


@pytest.mark.parametrize("case", ["horizontal-4", "directional-2"])
def test_gauge_ragged_shot_list_through_uneven_batches(tmp_path, hip_ops, probes_lib, case):
    """Three shots with DIFFERENT channel counts (all, a third, ONE) through the batched schedule with uneven sub-batches (two forward
    lanes for three shots, one backward lane) against the stream schedule: gathers and all five outputs bit for bit, as
    test_gauge_every_schedule_agrees has it for one backward lane; with a backward lane per shot the gradients to 5e-6 and misfit,
    source gradient and gathers bit for bit."""
    fiber, G = CASES[case]
    pb, fn, para = gauge_problem(tmp_path, fiber, G, nshots=3, src_x=[120, 250, 380], nSteps=360)
    sv = json.load(open(pb["survey_fname"]))
    n = sv["shot0"]["nrec"]
    for k, cnt in ((1, n // 3), (2, 1)):
        sh = sv["shot%d" % k]
        first = n // 2 if k == 2 else 0                      # the single channel in the middle of the line
        for key in ("z_rec", "x_rec") + (("das_sensitivity",) if "das_sensitivity" in sh else ()):
            sh[key] = sh[key][first:first + cnt]
        sh["nrec"] = cnt
    json.dump(sv, open(pb["survey_fname"], "w"))
    nS, ids = pb["nSteps"], pb["Shot_ids"]
    lt, mt, dt_ = pb["lame_true"]
    lam, mu, den = pb["lame_init"]
    lam = (lam * 1.05).contiguous()
    fwd, out = {}, {}
    for name, opts in (("streams", dict(batch=0)), ("uneven batches", dict(batch=1, batch_f=2, batch_b=1)), ("batched", dict(batch=1))):
        with P.kernel_options(**opts):
            hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, ids, fn)
            fwd[name] = {c: [ft.read_shot_gather(para["data_dir_name"], c, int(i), nS) for i in ids] for c in ("pr", "vx", "vz", "ett")}
            out[name] = [t.numpy().copy() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, ids, fn)]
    assert [a.shape[0] for a in fwd["streams"]["ett"]] == [n, n // 3, 1]
    assert out["streams"][0][0] > 0 and np.abs(out["streams"][1]).max() > 0 and all(np.abs(a).max() > 0 for a in fwd["streams"]["ett"])
    for name in ("uneven batches", "batched"):
        for c in fwd[name]:
            for i, (a, b) in enumerate(zip(fwd[name][c], fwd["streams"][c])):
                assert np.array_equal(a, b), (name, c, i)
    for k, (a, b) in enumerate(zip(out["uneven batches"], out["streams"])):
        assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))
    for k in (0, 4):
        assert np.array_equal(out["batched"][k], out["streams"][k]), k
    for k in (1, 2, 3):
        assert P.rel_l2(out["batched"][k], out["streams"][k]) <= 5e-6, k
