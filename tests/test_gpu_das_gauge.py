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
from sepfwi import _native
from sepfwi import utils as ft

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-3
CASES = {"horizontal-3": ("horizontal", 3), "horizontal-4": ("horizontal", 4), "vertical-3": ("vertical", 3), "directional-2": ("directional", 2)}


def members(G):
    """Members k and weights w_k of a gauge of G cells (midpoint rule for odd G, trapezoid rule for even G)."""
    if G % 2:
        ks = np.arange(-(G - 1) // 2, (G - 1) // 2 + 1)
        return ks, np.full(ks.size, 1.0 / G)
    ks = np.arange(-G // 2, G // 2 + 1)
    w = np.full(ks.size, 1.0 / G)
    w[0] = w[-1] = 0.5 / G
    return ks, w


def member_survey(survey, G, vertical):
    """Every channel c replaced by its members, channel-major (member j of channel c is channel c * M + j)."""
    ks, _ = members(G)
    out = {}
    for key, sh in survey.items():
        if not (key.startswith("shot") and key[4:].isdigit()):
            out[key] = sh
            continue
        z, x = np.asarray(sh["z_rec"]), np.asarray(sh["x_rec"])
        zm = (z[:, None] + (ks[None, :] if vertical else 0)) * np.ones((1, ks.size), int)
        xm = (x[:, None] + (0 if vertical else ks[None, :])) * np.ones((1, ks.size), int)
        new = dict(sh, z_rec=zm.ravel().tolist(), x_rec=xm.ravel().tolist(), nrec=int(zm.size))
        if "das_sensitivity" in sh:
            new["das_sensitivity"] = np.repeat(np.asarray(sh["das_sensitivity"]), ks.size, axis=0).tolist()
        out[key] = new
    return out


def gauge_of(member_ett, G):
    """(group, nrec * M, nSteps) member gathers -> (group, nrec, nSteps) gauge gathers, in float64."""
    _, w = members(G)
    g, n, nt = member_ett.shape
    return np.einsum("gcjt,j->gct", member_ett.reshape(g, n // w.size, w.size, nt).astype(np.float64), w)


def write_para(pb, name, **keys):
    """A parameter file next to pb's: same grid and survey, data directory <name>_Data, extra / changed keys."""
    para = dict(pb["para"], data_dir_name=os.path.join(os.path.dirname(pb["para_fname"]), name + "_Data"), **keys)
    os.makedirs(para["data_dir_name"], exist_ok=True)
    fn = os.path.join(os.path.dirname(pb["para_fname"]), name + ".json")
    with open(fn, "w") as fp:
        json.dump(para, fp)
    return fn, para


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
