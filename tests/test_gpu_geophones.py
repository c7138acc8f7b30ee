"""Joint DAS + geophone misfit (parameter keys "misfit_w_ett" / "misfit_w_vx" / "misfit_w_vz", csrc/geophone.{hpp,cpp,hip}) on the GPU,
through the C ABI: the vx / vz residuals enter misfit and adjoint source with their weights.

The oracle's driver injects the axial strain only; the reference here is tests/geophone_ref.py, the oracle's shot driver restated
over its exported kernels with the geophone adds (pinned to the oracle bit for bit by tests/test_geophone_reference.py).
Tolerances: the suite's -- misfit rtol 1e-4, gradients and gStf rel-L2 <= 1e-3 and max-norm <= 1e-3 max|g|."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import fuzz_common as FC
import geophone_ref as G
import problems as P
from sepfwi import _native
from sepfwi import utils as ft

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-3
COMPS = ("pr", "vx", "vz", "ett")
WEIGHTS = {"vx": (0.0, 1.0, 0.0), "vz": (0.0, 0.0, 1.0), "joint": (1.0, 0.5, 2.0)}     # (ett, vx, vz)
FIBERS = {"horizontal": {}, "vertical": dict(das_fiber="vertical"), "directional": dict(das_sensitivity="random", nrec_stride=2)}


write_para = functools.partial(FC.write_para, data_dir=None)      # pb's own data directory unless another is named


def write_obs(data_dir, ids, obs, comps=COMPS):
    os.makedirs(data_dir, exist_ok=True)
    for i, sid in enumerate(ids):
        for c in comps:
            np.ascontiguousarray(obs[i, COMPS.index(c)], dtype=np.float32).tofile(os.path.join(data_dir, "Shot_%s%d.bin" % (c, int(sid))))


def models(pb):
    lam, mu, den = pb["lame_init"]
    return pb["lame_true"], ((lam * 1.05).contiguous(), mu, den)        # residuals of the size of the data


def compare(tag, got, ref, parts, weights, nshots):
    dev = {"misfit": abs(float(got[0][0]) - ref["misfit"]) / ref["misfit"]}
    for k, key in ((1, "gLambda"), (2, "gMu"), (3, "gDen")):
        dev[key] = (P.rel_l2(got[k], ref[key]), float(np.abs(got[k] - ref[key]).max() / np.abs(ref[key]).max()))
    dev["gStf"] = P.rel_l2(got[4][:nshots], ref["gStf"])
    for c, w in zip(("ett", "vx", "vz"), weights):
        dev["part " + c] = abs(parts[c] - ref["parts"][c]) / ref["parts"][c] if w > 0 else parts[c]
    print("geophones %s: %r" % (tag, dev))
    assert ref["misfit"] > 0 and dev["misfit"] <= 1e-4, (tag, dev)
    for key in ("gLambda", "gMu", "gDen"):
        assert np.abs(ref[key]).max() > 0
        assert dev[key][0] <= GRAD_TOL and dev[key][1] <= GRAD_TOL, (tag, key, dev)
    assert np.abs(ref["gStf"]).max() > 0 and dev["gStf"] <= GRAD_TOL, (tag, dev)
    for c, w in zip(("ett", "vx", "vz"), weights):
        assert ref["parts"][c] > 0
        assert (dev["part " + c] <= 1e-4) if w > 0 else (parts[c] == 0.0), (tag, c, dev)    # a component without weight reports 0


@pytest.fixture(scope="module")
def small_cases(tmp_path_factory, oracle):
    """Per fibre kind the 50 x 90 problem, its observed gathers (oracle, true model) on disk, and the references of the weight sets --
    computed once, shared, left unchanged."""
    cache = {}

    def get(fiber, wname):
        if fiber not in cache:
            d = tmp_path_factory.mktemp("geo_" + fiber)
            pb = P.make_problem(str(d), nz=50, nx=90, nPml=10, nSteps=260, nshots=2, hetero=True, rec_z=30, **FIBERS[fiber])
            true, init = models(pb)
            obs = oracle.cufd(*[t.numpy() for t in true], pb["Stf"].numpy(), 2, pb["Shot_ids"].numpy(), pb["para"], pb["survey"])["syn"]
            write_obs(pb["data_dir"], pb["Shot_ids"].tolist(), obs)
            cache[fiber] = dict(pb=pb, obs=obs, init=init, refs={})
        c = cache[fiber]
        if wname not in c["refs"]:
            pb = c["pb"]
            c["refs"][wname] = G.cufd(oracle, *[t.numpy() for t in c["init"]], pb["Stf"].numpy(), 1, pb["Shot_ids"].numpy(), pb["para"], pb["survey"],
                                      obs=c["obs"], weights=WEIGHTS[wname])
        return c["pb"], c["init"], c["refs"][wname]

    return get


@pytest.mark.parametrize("fiber", sorted(FIBERS))
@pytest.mark.parametrize("wname", sorted(WEIGHTS))
def test_batched_schedule_matches_reference(small_cases, hip_ops, fiber, wname):
    """The batched schedule (batched residual kernel, k_inject_gauge_batch over the concatenated plan): geophones alone and jointly with
    a horizontal, a vertical and a directional fibre against geophone_ref; sepfwi_get_misfit_parts against the reference's sums."""
    pb, init, ref = small_cases(fiber, wname)
    fn, _ = write_para(pb, "w_" + wname, WEIGHTS[wname])
    with P.kernel_options(batch=1):
        got = [t.numpy().copy() for t in hip_ops.backward(*init, pb["Stf"], 1, pb["Shot_ids"], fn)]
        parts = hip_ops.misfit_parts(fn)
        assert hip_ops.stats(fn, 0)["persist_steps"] == 0
    compare("batched %s %s" % (fiber, wname), got, ref, parts, WEIGHTS[wname], 2)
    m = hip_ops.forward(*init, pb["Stf"], 0, pb["Shot_ids"], fn)[0]          # the misfit-only call forms the same residuals
    again = hip_ops.misfit_parts(fn)                                         # (double atomics: the order of the blocks' partial sums is free)
    assert abs(float(m[0]) - float(got[0][0])) <= 1e-6 * float(got[0][0]) and all(abs(again[c] - parts[c]) <= 1e-12 * parts[c] for c in parts)


@pytest.mark.parametrize("stride", [1, 3], ids=["line", "every-third"])
def test_loop_matches_reference_and_every_schedule_agrees(tmp_path, oracle, hip_ops, stride):
    """300 x 500 grid (2 880 row segments: enough for the persistent loop), weights (1, 0.5, 2): a consecutive line of channels -- sampled
    inside the forward kernels, vx and vz included, injected through the plan -- and a channel every third cell.  Every backward step
    runs inside the loop; results against geophone_ref; the two-launch step, the reference's launch structure and the batched schedule
    leave the same bits (one add per distinct target and step, folded in entry order, in all of them)."""
    w = WEIGHTS["joint"]
    pb = P.make_problem(str(tmp_path), nz=300, nx=500, nPml=10, nSteps=120, nshots=1, hetero=True, rec_z=8, nrec_stride=stride)
    true, init = models(pb)
    obs = oracle.cufd(*[t.numpy() for t in true], pb["Stf"].numpy(), 2, pb["Shot_ids"].numpy(), pb["para"], pb["survey"])["syn"]
    write_obs(pb["data_dir"], [0], obs)
    ref = G.cufd(oracle, *[t.numpy() for t in init], pb["Stf"].numpy(), 1, pb["Shot_ids"].numpy(), pb["para"], pb["survey"], obs=obs, weights=w)
    fn, _ = write_para(pb, "joint", w)
    out = {}
    for name, opts in (("loop", dict(batch=0, bwd_fuse=4)), ("two-launch", dict(batch=0, bwd_fuse=2)), ("reference launches", dict(batch=0, bwd_fuse=0)),
                       ("batched", dict(batch=1))):
        with P.kernel_options(**opts):
            out[name] = [t.numpy().copy() for t in hip_ops.backward(*init, pb["Stf"], 1, pb["Shot_ids"], fn)]
            steps = hip_ops.stats(fn, 0)["persist_steps"]
            assert steps == (pb["nSteps"] - 1 if name == "loop" else 0), (name, steps, hip_ops.loop_status(fn))
            if name == "loop":
                parts = hip_ops.misfit_parts(fn)
    compare("loop stride %d" % stride, out["loop"], ref, parts, w, 1)
    for name in ("two-launch", "reference launches", "batched"):
        for k, (a, b) in enumerate(zip(out[name], out["loop"])):
            assert np.array_equal(a, b), (name, k, float(np.abs(a - b).max()))


def test_geophones_compose_with_the_gauge(tmp_path, hip_ops):
    """das_gauge_length = 3 dx plus geophones: the gradient is linear in the adjoint source for a fixed model, so the joint call equals
    the sum of the three calls with one component each (the gauge-only one is pinned by the gauge tests, the geophone-only ones by the
    tests above) within the gradient tolerance, and its misfit their sum to 1e-6."""
    pb = P.make_problem(str(tmp_path), nz=50, nx=90, nPml=10, nSteps=260, nshots=2, hetero=True, rec_z=30)
    true, init = models(pb)
    L3 = 3 * pb["para"]["dx"]
    fn_obs, _ = write_para(pb, "observe", das_gauge_length=L3)
    hip_ops.obscalc(*true, pb["Stf"], 1, pb["Shot_ids"], fn_obs)             # gauge ett, vx, vz of the true model -> the shared data directory
    w = WEIGHTS["joint"]
    runs = {}
    for name, ws in (("joint", w), ("ett", (w[0], 0.0, 0.0)), ("vx", (0.0, w[1], 0.0)), ("vz", (0.0, 0.0, w[2]))):
        fn, _ = write_para(pb, "gauge_" + name, ws, das_gauge_length=L3)
        runs[name] = [t.numpy().astype(np.float64) for t in hip_ops.backward(*init, pb["Stf"], 1, pb["Shot_ids"], fn)]
    total = [runs["ett"][k] + runs["vx"][k] + runs["vz"][k] for k in range(5)]
    assert all(runs[n][0][0] > 0 and np.abs(runs[n][3]).max() > 0 for n in runs)
    assert abs(runs["joint"][0][0] - total[0][0]) <= 1e-6 * total[0][0], (runs["joint"][0], total[0])
    for k in (1, 2, 3, 4):
        dev = (P.rel_l2(runs["joint"][k], total[k]), float(np.abs(runs["joint"][k] - total[k]).max() / np.abs(total[k]).max()))
        print("gauge + geophones, output %d: %r" % (k, dev))
        assert dev[0] <= GRAD_TOL and dev[1] <= GRAD_TOL, (k, dev)


def test_default_weights_change_nothing(tmp_path, hip_ops):
    """Keys (1, 0, 0) against no keys: misfit, gradients, gStf bit-identical, persist_steps and launch count equal -- the path that always
    ran, the fused line inside the field kernels included.  paraGen without misfit_weights writes the bytes it always wrote."""
    pb = P.make_problem(str(tmp_path), nz=300, nx=500, nPml=10, nSteps=120, nshots=2, hetero=True, rec_z=8)
    true, init = models(pb)
    hip_ops.obscalc(*true, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    fn, _ = write_para(pb, "explicit", (1.0, 0.0, 0.0))
    res = {}
    for name, f in (("absent", pb["para_fname"]), ("explicit", fn)):
        with P.kernel_options(batch=0):                                          # one loop per shot, the line fused into the field kernels
            out = [t.numpy().copy() for t in hip_ops.backward(*init, pb["Stf"], 1, pb["Shot_ids"], f)]
            st = hip_ops.stats(f, 0)
            res[name] = (out, st["persist_steps"], st["launches"], hip_ops.misfit_parts(f))
    assert res["absent"][0][0][0] > 0 and res["absent"][1] == 2 * (pb["nSteps"] - 1)
    for k in range(5):
        assert np.array_equal(res["absent"][0][k], res["explicit"][0][k]), k
    assert res["absent"][1:3] == res["explicit"][1:3], (res["absent"][1:], res["explicit"][1:])
    p = res["absent"][3]
    assert res["explicit"][3]["ett"] == p["ett"] or abs(res["explicit"][3]["ett"] - p["ett"]) <= 1e-12 * p["ett"]
    assert p["vx"] == 0.0 and p["vz"] == 0.0 and abs(p["ett"] - float(res["absent"][0][0][0])) <= 1e-6 * p["ett"]
    a, b = os.path.join(str(tmp_path), "a.json"), os.path.join(str(tmp_path), "b.json")
    args = (60, 80, 10.0, 10.0, 100, 1e-3, 10.0, 10, 2)
    ft.paraGen(*args, a, "s.json", os.path.join(str(tmp_path), "D"))
    ft.paraGen(*args, b, "s.json", os.path.join(str(tmp_path), "D"), misfit_weights=None)
    assert open(a, "rb").read() == open(b, "rb").read() and b"misfit_w" not in open(a, "rb").read()


def test_every_data_route_gives_the_same_bits(tmp_path, hip_ops):
    """Observed vx / vz / ett from the Shot_* files, from sepfwi_set_observed_component, from calc_id 3 (the store) and under an HBM budget
    small enough to evict (pinned-host tier, three gathers per shot): all five outputs bit-identical.  Weights (0, 1, 1) run without
    any Shot_ett file on disk."""
    pb = P.make_problem(str(tmp_path), nz=50, nx=90, nPml=10, nSteps=300, nshots=4, hetero=True, rec_z=30)
    true, init = models(pb)
    ids, nS, w = pb["Shot_ids"], pb["nSteps"], WEIGHTS["joint"]
    fn_files, _ = write_para(pb, "files", w)
    hip_ops.obscalc(*true, pb["Stf"], 1, ids, fn_files)                         # calc_id 2: the four files per shot

    def run(f):     # one launch structure for every route: the stream schedule sums every shot into one set of accumulators in shot order,
        with P.kernel_options(batch=0):     # whatever group size the budget leaves (a batch's lanes are summed at the end, per lane)
            return [t.numpy().copy() for t in hip_ops.backward(*init, pb["Stf"], 1, ids, f)]

    out = {"files": run(fn_files)}
    fn_mem, _ = write_para(pb, "memory", w, data_dir="Empty_memory")
    for sid in ids.tolist():
        for c in ("vx", "vz", "ett"):
            hip_ops.set_observed_component(fn_mem, sid, c, torch.from_numpy(ft.read_shot_gather(pb["data_dir"], c, sid, nS).copy()))
    out["memory"] = run(fn_mem)
    fn_store, _ = write_para(pb, "store", w, data_dir="Empty_store")
    hip_ops.obscalc(*true, pb["Stf"], 1, ids, fn_store, to_store=True)           # calc_id 3: every component with a weight
    out["store"] = run(fn_store)
    assert os.listdir(os.path.join(str(tmp_path), "Empty_store")) == [] and os.listdir(os.path.join(str(tmp_path), "Empty_memory")) == []
    fn_evict, _ = write_para(pb, "evict", w, obs_cache_mb=1)                     # 12 gathers of 98 kB against 1 MB
    out["evict"] = run(fn_evict)
    st = hip_ops.stats(fn_evict, 0)
    assert st["obs_evictions"] > 0 and st["obs_host_bytes"] > 0, st
    out["evict again"] = run(fn_evict)                                           # gathers that return from the host tier
    assert out["files"][0][0] > 0 and np.abs(out["files"][1]).max() > 0
    for name in out:
        for k in range(5):
            assert np.array_equal(out[name][k], out["files"][k]), (name, k)
    only = os.path.join(str(tmp_path), "Only_geophones")
    os.makedirs(only)
    for sid in ids.tolist():
        for c in ("vx", "vz"):
            ft.read_shot_gather(pb["data_dir"], c, sid, nS).tofile(os.path.join(only, "Shot_%s%d.bin" % (c, sid)))
    fn_geo, _ = write_para(pb, "geophones_only", (0.0, 1.0, 1.0), data_dir="Only_geophones")
    geo = run(fn_geo)
    parts = hip_ops.misfit_parts(fn_geo)
    assert geo[0][0] > 0 and parts["ett"] == 0.0 and abs(parts["vx"] + parts["vz"] - float(geo[0][0])) <= 1e-6 * float(geo[0][0])


REFUSALS = {
    "pack + vx": (dict(misfit_w_vx=1.0, obs_pack_fname="pack.bin"), -1, ("misfit_w_vx", "obs_pack_fname")),
    "pack + vz": (dict(misfit_w_vz=1.0, obs_pack_fname="pack.bin"), -1, ("misfit_w_vz", "obs_pack_fname")),
    "if_win": (dict(misfit_w_vx=1.0, if_win=True), -1, ("misfit_w_vx", "if_win")),
    "filter": (dict(misfit_w_vz=2.0, filter=[3.0, 7.0, 40.0, 60.0]), -1, ("misfit_w_vz", "filter")),
    "if_cross_misfit": (dict(misfit_w_vx=0.5, if_cross_misfit=True), -1, ("misfit_w_vx", "if_cross_misfit")),
    "if_src_update": (dict(misfit_w_vz=0.5, if_src_update=True), -1, ("misfit_w_vz", "if_src_update")),
    "negative": (dict(misfit_w_vx=-1.0), -5, ("misfit_w_vx",)),
    "not a number": (dict(misfit_w_vz="2"), -5, ("misfit_w_vz",)),
    "all zero": (dict(misfit_w_ett=0.0), -5, ("misfit_w_ett", "misfit_w_vx", "misfit_w_vz")),
    "missing file": (dict(misfit_w_vz=1.0), -2, ("Shot_vz0.bin",)),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_reach_the_c_abi(tmp_path, hip_ops, name):
    """Every refused combination returns its code through the C ABI and its message names the key (or the missing file); the same
    live-conditioning key with "conditioning": "reference" is parsed and ignored, so it stays allowed."""
    keys, code, words = REFUSALS[name]
    pb = P.make_problem(str(tmp_path), nz=40, nx=48, nPml=10, nSteps=60, nshots=1, hetero=False)
    true, init = models(pb)
    hip_ops.obscalc(*true, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    if name == "missing file":
        os.remove(os.path.join(pb["data_dir"], "Shot_vz0.bin"))
    fn, _ = write_para(pb, "refused", **keys)
    with pytest.raises(_native.SepFwiError) as e:
        hip_ops.forward(*init, pb["Stf"], 0, pb["Shot_ids"], fn)
    assert e.value.code == code, str(e.value)
    for wd in words:
        assert wd in str(e.value), str(e.value)
    if name in ("filter", "if_cross_misfit"):
        fn_ref, _ = write_para(pb, "reference_mode", conditioning="reference", **keys)
        assert float(hip_ops.forward(*init, pb["Stf"], 0, pb["Shot_ids"], fn_ref)[0][0]) > 0
    assert float(hip_ops.forward(*init, pb["Stf"], 0, pb["Shot_ids"], pb["para_fname"])[0][0]) > 0 or name == "missing file"   # the library is fine afterwards


def test_component_and_parts_entry_points_check_their_arguments(tmp_path, hip_ops):
    """sepfwi_set_observed_component: comp 0 and 4 are SEPFWI_EINVAL, comp 3 is sepfwi_set_observed; sepfwi_get_misfit_parts without a
    session is SEPFWI_EINVAL like the other queries."""
    pb = P.make_problem(str(tmp_path), nz=40, nx=48, nPml=10, nSteps=60, nshots=1, hetero=False)
    L = _native.lib()
    fn = pb["para_fname"].encode()
    data = np.zeros((pb["nrec"], pb["nSteps"]), np.float32)
    ptr = C.c_void_p(data.ctypes.data)
    parts = (C.c_double * 3)()
    hip_ops.release()
    assert L.sepfwi_get_misfit_parts(fn, 0, parts) == -1 and b"no session" in L.sepfwi_last_error()
    for comp in (0, 4, -1):
        assert L.sepfwi_set_observed_component(fn, 0, 0, comp, ptr, pb["nrec"], pb["nSteps"]) == -1
        assert b"comp" in L.sepfwi_last_error()
    for comp in (1, 2, 3):
        assert L.sepfwi_set_observed_component(fn, 0, 0, comp, ptr, pb["nrec"], pb["nSteps"]) == 0
    assert L.sepfwi_set_observed_component(fn, 0, 0, 1, ptr, pb["nrec"] + 1, pb["nSteps"]) == -1
    assert L.sepfwi_get_misfit_parts(fn, 0, parts) == 0 and list(parts) == [0.0, 0.0, 0.0]
    true, init = models(pb)
    m = hip_ops.forward(*init, pb["Stf"], 0, pb["Shot_ids"], pb["para_fname"])[0]          # zero observed ett from memory: r = -syn
    assert float(m[0]) > 0 and abs(hip_ops.misfit_parts(pb["para_fname"])["ett"] - float(m[0])) <= 1e-6 * float(m[0])
