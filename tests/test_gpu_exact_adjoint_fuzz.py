"""Seeded random small problems for the exact discrete adjoint: HIP (csrc/exact_adjoint.hip, csrc/session_exact.cpp, sepfwi_adjoint_exact)
against J itself outside the GPU (-m gpu).  tests/test_gpu_exact_adjoint.py holds the pass on hand-picked problems; this file holds it
where those do not reach: channels INSIDE the absorbing layers (the order of injection and k_exact_b, the priming of Q for column
nSteps-1), the column where the x strips of S and V differ, ragged channel counts with the caller's w, w in host memory, the exact
gradient of a joint / gauge / ragged misfit (k_geo_residual), padded widths below 64, layer widths 4 ... 12, nPad 0 ... 8 with dz != dx,
a water layer, and a session whose earlier call left quiet maps behind.

Every seed is a draw of tests/test_gpu_fuzz.py (draw_problem) changed by tests/test_gpu_born_fuzz.py (draw_born: conditioning keys
removed, option set, ragged counts, joint weights, gauge G 2 ... 5) and then by draw_exact from a generator of its own
(default_rng(EXACT_SEED0 + seed); every quantity is drawn for every seed, used or not, so the geometry of a seed stays what the other fuzz
files see):
  * LAYER MODE in one draw of three, never on a gauge draw: the channel lists of all shots are replaced as a whole by 6 ... 12 channels
    inside the absorbing strips, on update cells [2, n-3] only: the top strip (rows 2 ... nPml-1, any column), the left strip (columns
    2 ... nPml-1) and the right strip (columns nx_pad-nPml ... nx_pad-3), rows of the upper half of the grid for left and right; the
    first three channels are one per strip, the third on padded column nx_pad-nPml exactly (inside the strip of S, outside that of V);
    the others fall uniformly on the three, but on a directional draw the last one sits on padded column nx_pad-3, the last of the update
    region (its exz term reaches column nx_pad-2 outside it, as a channel on row or column 2 reaches row or column 1).  Survey coordinates are padded minus nPml, so they may be negative.  No channel in the bottom
    strip and none in the interior: within these record lengths a bottom channel carries 1e-4 ... 1e-6 of the others' amplitude, and layer
    channels mixed into an interior line 1e-2 ... 1e-1 of the gather -- an error of order 1 in them would drown.  The misfit is the joint
    one, weights (1, w_vx, w_vz) with draw_born's own w_vx, w_vz, so that velocities are injected in the layers (Q); directional draws
    get sensitivities for the new channels; ragged counts are drawn again for the new list and applied after the replacement.
  * three perturbations, all masked to Omega and with dMu = 0 in water rows: v = smooth + white noise (exact_adjoint_ref.smooth_v,
    white_v, two seeds), d = lame_true - lame_init (J d is the linearised residual: cos(J d, r) 0.9 ... 1.0, where a smooth v is
    orthogonal to r on half of the draws and would decide nothing about the gradient).

Reference (oracle_side, no GPU; tests/test_exact_adjoint_fuzz_reference.py runs it on the default seeds): per oracle build three runs of
tests/born_ref.py through test_gpu_born_fuzz.born_side -- (m_init, v): syn and J v; (m_init, d): J d; (m_true, 0): obs -- and
r = obs - syn in float64, obs rounded to float32 as it is installed.  All dot products in float64.  Tolerances are those of
tests/test_gpu_exact_adjoint.py (held, TOL = 1e-3, 3 x the difference of the same quantity between the two oracle builds), none new:
    v^T H v       against |W^1/2 J_ref v|^2 (scale |ref|), and against the GPU's own born gathers (yardstick 0)
    <v, J^T w>    w_c = W_c (J_ref d)_c in float32, against <J_ref v, w> = <W J_ref v, J_ref d>, scale |W^1/2 J v| |W^1/2 J d| (the cosine
                  of such pairs runs from -0.5 to 0.9 and is sometimes about 0); device tensors and host memory through the C ABI give
                  the same bits; with more than one shot the last shot alone (ids = [last], its own count, its w at offset 0) on that
                  shot's own scale -- the last shot whose own record is live, where the very last one's is not
    <g, d>        exact gradient of the misfit with obs installed per shot and weighted component, against <J_ref d, -W r>:
                  (1e-3 + cond_g) |ref| + 3 |alt - ref|, cond_g = 4 eps sqrt(E / misfit) of tests/test_gpu_fuzz.py (the GPU forms r from
                  its own float32 syn)
A draw on which the yardstick of any comparison exceeds 1e-2 of its scale, or cond_g > 1e-2, has no target and is reported as xfail.
A draw whose record is not live -- the wave misses the channels, a layer channel stays below 1e-3 of the largest, or cond_g > 1e-2 because
the wave has not come back from where the models differ -- is drawn again with the record two, then four times as long (oracle_side);
still not live then, it is an xfail too.
profiles/r12_exact_adjoint_fuzz.txt holds the deviations measured on the MI355X and what the fuzz does to five deliberately wrong
variants of the pass."""
import json
import os

import numpy as np
import pytest
import torch

import born_ref as B
import exact_adjoint_ref as X
import problems as P
import test_gpu_born_fuzz as BF
import test_gpu_exact_adjoint as G
import test_gpu_fuzz as F

pytestmark = pytest.mark.gpu

EXACT_SEED0 = 95400
COMPS = BF.COMPS
TOL = G.TOL
MAX_LAYER_CHANNELS = 12

_SEEDS = ([int(v) for v in os.environ["SEPFWI_EXACT_FUZZ_SEEDS"].split(",")] if os.environ.get("SEPFWI_EXACT_FUZZ_SEEDS")
          else list(range(int(os.environ.get("SEPFWI_EXACT_FUZZ_N", "16")))))


def born_weights(seed):
    """(w_vx, w_vz) as draw_born draws them for every seed (it returns them only where it uses them): its generator replayed."""
    rg = np.random.default_rng(BF.BORN_SEED0 + seed)
    rg.integers(0, 4), rg.integers(0, len(BF.OPTION_SETS)), rg.integers(0, 2), rg.integers(0, 4)
    w_vx, w_vz = [float(np.round(w, 3)) for w in rg.uniform(0.1, 1.0, 2)]
    return w_vx, w_vz


def strips(pb):
    """{name: (rows lo..hi, columns lo..hi)} of the three strips of layer mode, padded cells, inclusive"""
    nPml, nzc, nx = pb["nPml"], pb["nz_pad"] - pb["nPad"], pb["nx_pad"]
    half = max(nPml, nzc // 2)
    return dict(top=((2, nPml - 1), (2, nx - 3)), left=((2, half), (2, nPml - 1)), right=((2, half), (nx - nPml, nx - 3)))


def draw_exact(d, b, seed):
    """Changes the draw (d: draw_problem, b: draw_born) as the module docstring says, rewrites its two files and updates b (counts,
    ragged, weights).  -> dict(layer, cells (padded (z, x) of the layer channels, else None), v_seeds)."""
    pb, sv = d["pb"], d["sv"]
    nPml = pb["nPml"]
    nshots = int(pb["Shot_ids"].numel())
    rg = np.random.default_rng(EXACT_SEED0 + seed)
    layer = int(rg.integers(0, 3)) == 0 and not b["G"]
    m = int(rg.integers(6, MAX_LAYER_CHANNELS + 1))
    place = [0, 1, 2] + [int(p) for p in rg.integers(0, 3, size=MAX_LAYER_CHANNELS - 3)]
    u = rg.uniform(size=(MAX_LAYER_CHANNELS, 2))
    sens = rg.uniform(-1.0, 1.0, (MAX_LAYER_CHANNELS, 3))
    cu = rg.uniform(size=4)
    single = int(rg.integers(0, 4)) % nshots
    v_seeds = [int(s) for s in rg.integers(0, 2 ** 31, size=2)]
    cells = None
    if layer:
        st = strips(pb)
        cells = []
        directional = "das_sensitivity" in sv["shot0"]
        if directional:     # the last channel on the LAST column of the update region: a directional channel reaches column x+1 outside it
            place[m - 1] = 2
        for k in range(m):
            (z0, z1), (x0, x1) = st[("top", "left", "right")[place[k]]]
            z, x = z0 + int(u[k, 0] * (z1 - z0 + 1)), x0 + int(u[k, 1] * (x1 - x0 + 1))
            if k == 2:
                x = pb["nx_pad"] - nPml      # the column inside the x strip of S and outside that of V
            if directional and k == m - 1:
                x = pb["nx_pad"] - 3
            cells.append((min(z, z1), min(x, x1)))
        counts = [min(m, 1 + int(c * m)) for c in cu[:nshots]]
        if b["ragged"]:     # (draw_born: more than one shot) a single-channel shot and one with the whole list
            counts[single], counts[(single + 1) % nshots] = 1, m
        else:
            counts = [m] * nshots
        for k in range(nshots):
            sh = sv["shot%d" % k]
            directional = "das_sensitivity" in sh
            n = counts[k]
            sh["z_rec"], sh["x_rec"], sh["nrec"] = [int(z - nPml) for z, _ in cells[:n]], [int(x - nPml) for _, x in cells[:n]], n
            if directional:
                full = np.zeros((n, 6))
                full[:, [0, 3, 1]] = sens[:n]
                sh["das_sensitivity"] = full.tolist()
        w_vx, w_vz = born_weights(seed)
        para = dict(pb["para"], misfit_w_ett=1.0, misfit_w_vx=w_vx, misfit_w_vz=w_vz)
        b.update(counts=counts, weights=(1.0, w_vx, w_vz))
        json.dump(sv, open(pb["survey_fname"], "w"))
        json.dump(para, open(pb["para_fname"], "w"))
        pb["para"] = para
    return dict(layer=layer, cells=cells, v_seeds=v_seeds)


def perturbations(d, e):
    """v and d of the module docstring -> two lists of three float32 (nz_pad, nx_pad) arrays"""
    pb, w = d["pb"], d["water"]
    v = [B.f32(a + c) for a, c in zip(X.smooth_v(pb, e["v_seeds"][0], w), X.white_v(pb, e["v_seeds"][1], w))]
    dm = [t.numpy() - i.numpy() for t, i in zip(pb["lame_true"], pb["lame_init"])]
    dm[1][:int(w)] = 0.0
    return v, X.on_omega(pb, dm)


def wdot(a, b, weights, shots=None):
    """sum over shots (all, or those listed) and weighted components of w_c <a_c, b_c>, float64; a, b: per shot {component: array}
    (a component that b does not hold counts as 0)"""
    shots = range(len(a)) if shots is None else shots
    return sum(w * float((np.asarray(a[i][c], np.float64) * np.asarray(b[i][c], np.float64)).sum()) for i in shots for c, w in zip(COMPS, weights)
               if w > 0 and c in b[i])


def channel_peaks(syn, b):
    """{(component, channel): the channel's own peak over all shots that hold it / the largest of that component's gathers} for the
    components that carry a weight; syn: per shot {component: (nrec, nSteps)}"""
    out = {}
    for c, wc in zip(COMPS, b["weights"] or (1.0, 0.0, 0.0)):
        if wc > 0:
            pk = np.zeros(max(b["counts"]))
            for s in syn:
                p = np.abs(np.asarray(s[c], np.float64)).max(axis=1)
                pk[:p.size] = np.maximum(pk[:p.size], p)
            out.update({(c, ch): float(p / max(pk.max(), 1e-300)) for ch, p in enumerate(pk)})
    return out


def build_side(lib, pb, sv, b, m_init, m_true, v, dm, one, first=None):
    """Everything one oracle build says about the draw.  one: the shot of the single-shot case; first: born_side(m_init, v) where the
    caller has run it already."""
    weights = b["weights"] or (1.0, 0.0, 0.0)
    syn, jv, raw = first or BF.born_side(lib, pb, sv, b, m_init, v)
    _, jd, _ = BF.born_side(lib, pb, sv, b, m_init, dm)
    obs, _, _ = BF.born_side(lib, pb, sv, b, m_true, [np.zeros_like(a) for a in v])
    obs = [{c: np.ascontiguousarray(o[c], dtype=np.float32) for c in COMPS} for o in obs]      # what is installed
    r = [{c: o[c].astype(np.float64) - np.asarray(s[c], np.float64) for c in COMPS} for o, s in zip(obs, syn)]
    w = [{c: np.ascontiguousarray(wc * np.asarray(q[c], np.float64), dtype=np.float32) for c, wc in zip(COMPS, weights) if wc > 0} for q in jd]
    unit = (1.0, 1.0, 1.0)
    return dict(syn=syn, jv=jv, jd=jd, obs=obs, r=r, w=w, raw=raw,
                nv=wdot(jv, jv, weights), nd=wdot(jd, jd, weights), vw=wdot(jv, w, unit), vw_one=wdot(jv, w, unit, [one]),
                nv_one=wdot(jv, jv, weights, [one]), nd_one=wdot(jd, jd, weights, [one]),
                gd=-wdot(jd, r, weights), misfit=0.5 * wdot(r, r, weights), E=0.5 * wdot(obs, obs, weights),
                cos_dr=wdot(jd, r, weights) / max(np.sqrt(wdot(jd, jd, weights) * wdot(r, r, weights)), 1e-300))


def oracle_side(tmp_path, oracle, oracle_nvfma, seed, scale):
    """The draw and everything the two oracle builds say about it (no GPU).  -> None when the record is not live (the caller draws again
    with a longer record), else a dict; ["target"] is False where a comparison has no target.  Three things count as 'not live', all of
    them a record that ends too early: the wave has not reached the channels (the precursor criterion of test_gpu_fuzz.py); on a layer
    draw it has not reached every strip (a channel's peak below 1e-3 of the largest decides nothing); it has not come back from where
    lame_true and lame_init differ (r holds rounding only: cond_g > 1e-2).  A draw that is still not live with four times the record
    is reported as xfail like any draw without a target, never passed."""
    d = F.draw_problem(tmp_path, seed, scale)
    b = BF.draw_born(d, seed)
    e = draw_exact(d, b, seed)
    pb, sv = d["pb"], d["sv"]
    m_init, m_true = [t.numpy() for t in pb["lame_init"]], [t.numpy() for t in pb["lame_true"]]
    v, dm = perturbations(d, e)
    first = BF.born_side(oracle, pb, sv, b, m_init, v)
    src_scale = float(np.abs(pb["Stf"].numpy()).max()) * 1500.0 ** 2 * float(pb["para"]["dt"])
    peak = max(float(np.abs(s["ett"]).max()) for s in first[0])
    if peak < 3e-10 * src_scale:      # only the stencil's numerical precursor (test_gpu_fuzz.py)
        return None
    if e["layer"] and min(channel_peaks(first[0], b).values()) < 1e-3:      # a strip the wave has not reached yet: a channel that decides nothing
        return None
    # the single-shot case: the last shot whose own record is live by the same criterion (seed 10: the last shot's gathers are 1e-15 of
    # the draw's, the stencil's precursor only, and its own |J v| |J d| is no scale for any float32 pass; the shot before it is taken)
    one = max(i for i, s in enumerate(first[0]) if float(np.abs(s["ett"]).max()) >= 3e-10 * src_scale)
    ref = build_side(oracle, pb, sv, b, m_init, m_true, v, dm, one, first)
    cond_g = 4.0 * 2.0 ** -24 * float(np.sqrt(ref["E"] / max(abs(ref["misfit"]), 1e-300)))
    if cond_g > 1e-2:       # the wave has not come back from where the two models differ: r holds rounding only, as above for the gather
        return None
    alt = build_side(oracle_nvfma, pb, sv, b, m_init, m_true, v, dm, one)
    # the comparisons: (reference, the other build's, scale)
    cmp = {"vHv": (ref["nv"], alt["nv"], abs(ref["nv"])),
           "<v,JTw>": (ref["vw"], alt["vw"], float(np.sqrt(ref["nv"] * ref["nd"]))),
           "<g,d>": (ref["gd"], alt["gd"], abs(ref["gd"]))}
    if len(ref["jv"]) > 1:
        cmp["<v,JTw> one shot"] = (ref["vw_one"], alt["vw_one"], float(np.sqrt(ref["nv_one"] * ref["nd_one"])))      # the shot's OWN scale
    yard = {k: abs(a - r) / max(s, 1e-300) for k, (r, a, s) in cmp.items()}
    target = all(s > 0 and y <= 1e-2 for (_, _, s), y in zip(cmp.values(), yard.values())) and cond_g <= 1e-2
    return dict(d=d, b=b, e=e, m=m_init, v=v, dm=dm, ref=ref, alt=alt, cmp=cmp, yard=yard, cond_g=cond_g, target=target, one=one)


def describe(o, scale):
    e = o["e"]
    return BF.describe(o, scale) + (", LAYER channels %r" % (e["cells"],) if e["layer"] else "")


# ---- the GPU side ------------------------------------------------------------------------------------------------------------
def _np(ts):
    return [t.cpu().numpy() for t in ts]


def flat_w(ref):
    """the caller's w as sepfwi_adjoint_exact takes it: per component one [nrec_i][nSteps] block per shot, shot after shot (or None)"""
    return [np.concatenate([w[c].reshape(-1) for w in ref["w"]]) if c in ref["w"][0] else None for c in COMPS]


def gpu_calls(hip_ops, o, with_plain=True):
    """Every call of the draw in one session, observed data installed first -> dict of numpy results"""
    d, b, ref = o["d"], o["b"], o["ref"]
    pb = d["pb"]
    fn, stf, ids = pb["para_fname"], pb["Stf"], pb["Shot_ids"]
    weights = b["weights"] or (1.0, 0.0, 0.0)
    m, v = G.cuda(o["m"]), G.cuda(o["v"])
    out = {}
    out["hv"] = _np(hip_ops.gauss_newton(*m, *v, stf, 1, ids, fn, exact=True))
    out["own"] = [{c: g[c].cpu().numpy() for c in COMPS} for g in hip_ops.born(*m, *v, stf, 1, ids, fn, components=COMPS)]
    w = [{c: torch.from_numpy(a).cuda() for c, a in sh.items()} for sh in ref["w"]]
    out["jtw"] = _np(hip_ops.born_adjoint(*m, w, stf, 1, ids, fn))
    rc, out["jtw_host"] = G.capi(pb, fn, [np.ascontiguousarray(a, dtype=np.float32) for a in o["m"]], w=flat_w(ref), host_out=True)
    assert rc == 0, rc
    if len(w) > 1:      # one shot alone: ids = [that shot], its own channel count, its w at offset 0
        k = o["one"]
        out["jtw_one"] = _np(hip_ops.born_adjoint(*m, w[k:k + 1], stf, 1, ids[k:k + 1], fn))
    for i, sid in enumerate(ids.tolist()):
        for c, wc in zip(COMPS, weights):
            if wc > 0:
                hip_ops.set_observed_component(fn, sid, c, torch.from_numpy(ref["obs"][i][c]))
    if with_plain:
        out["plain"] = _np(hip_ops.backward(*m, stf, 1, ids, fn))
        out["parts"] = hip_ops.misfit_parts(fn)
    ex = hip_ops.backward(*m, stf, 1, ids, fn, exact_adjoint=True)
    assert len(ex) == 5 and not torch.any(ex[4])
    out["exact"] = _np(ex[:4])
    out["status"] = hip_ops.loop_status(fn)
    if with_plain:
        out["parts_after"] = hip_ops.misfit_parts(fn)
        out["plain_after"] = _np(hip_ops.backward(*m, stf, 1, ids, fn))
    return out


EXACT_KEYS = ("hv", "jtw", "jtw_host", "jtw_one", "exact")


def same_bits(a, b, what, keys=EXACT_KEYS + ("plain", "plain_after")):
    for k in keys:
        if k in a or k in b:
            assert len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), (what, k)
    for i, (x, y) in enumerate(zip(a["own"], b["own"])):
        assert all(np.array_equal(x[c], y[c]) for c in COMPS), (what, "born gathers of shot %d" % i)


@pytest.mark.parametrize("seed", _SEEDS)   # one-off sweeps: SEPFWI_EXACT_FUZZ_N=100 (CPU-oracle bound)
def test_random_problem_matches_oracle_exact_adjoint(tmp_path, oracle, oracle_nvfma, hip_ops, seed):
    """As test_random_problem_matches_oracle: a draw whose record ends before the wave reaches the channels is drawn again with the
    record two, then four times as long."""
    for scale in (1, 2, 4):
        if _attempt(tmp_path / ("x%d" % scale), oracle, oracle_nvfma, hip_ops, seed, scale):
            return
    pytest.xfail("seed %d: the record is not live even when four times as long (the wave does not reach the channels or every strip of a "
                 "layer draw, or the residual holds rounding only: oracle_side)" % seed)


def _attempt(tmp_path, oracle, oracle_nvfma, hip_ops, seed, scale):
    from sepfwi import fwi_ops
    o = oracle_side(tmp_path, oracle, oracle_nvfma, seed, scale)
    if o is None:
        return False
    d, b, ref, alt = o["d"], o["b"], o["ref"], o["alt"]
    pb, opts, water = d["pb"], b["opts"], d["water"]
    fn = pb["para_fname"]
    tag = "exact fuzz seed %d (%s)" % (seed, describe(o, scale))
    weights = b["weights"] or (1.0, 0.0, 0.0)
    omega = X.mask_omega(pb)
    fwi_ops.release()
    with P.kernel_options(**opts):      # 4. every GPU call under the draw's options
        if opts.get("quiet_skip"):
            # a plain misfit call with quiet_skip = 1 first: it leaves quiet maps behind in the session that then serves the exact pass
            hip_ops.obscalc(*[t.cuda() for t in pb["lame_true"]], pb["Stf"], 1, pb["Shot_ids"], fn)
            hip_ops.forward(*G.cuda(o["m"]), pb["Stf"], 0, pb["Shot_ids"], fn)
        first = gpu_calls(hip_ops, o)
        same_bits(first, gpu_calls(hip_ops, o), (tag, "second call of the session"))
    if opts.get("quiet_skip"):      # ... and a fresh session that never saw quiet_skip gives the exact pass's bits
        fwi_ops.release()
        with P.kernel_options(quiet_skip=0):
            same_bits(first, gpu_calls(hip_ops, o, with_plain=False), (tag, "fresh session with quiet_skip = 0"), keys=EXACT_KEYS)
    fwi_ops.release()

    got = {"vHv": X.model_dot(o["v"], first["hv"]), "<v,JTw>": X.model_dot(o["v"], first["jtw"]), "<g,d>": X.model_dot(o["dm"], first["exact"][1:])}
    if "jtw_one" in first:
        got["<v,JTw> one shot"] = X.model_dot(o["v"], first["jtw_one"])
    own = wdot(first["own"], first["own"], weights)
    cond_g = o["cond_g"]
    line = {k: "%.2e (builds %.2e)" % (abs(got[k] - r) / max(s, 1e-300), o["yard"][k]) for k, (r, a, s) in o["cmp"].items()}
    line["vHv against own J v"] = "%.2e" % (abs(got["vHv"] - own) / max(abs(own), 1e-300))
    line["cond_g"] = "%.1e" % cond_g
    if "jtw_one" in first:
        line["the one shot"] = "%d of %d" % (o["one"], len(first["own"]))
    line["cos(Jd, r)"] = "%.3f" % ref["cos_dr"]
    line["cos(Jv, Jd)"] = "%.3f" % (ref["vw"] / max(o["cmp"]["<v,JTw>"][2], 1e-300))
    print("%s: %r" % (tag, line))
    if not o["target"]:
        pytest.xfail("seed %d: no target -- the two oracle builds differ by %r of the scales (conditioning term %.1e)" % (seed, o["yard"], cond_g))

    # 1. the Gauss-Newton product
    G.outside_is_zero(pb, first["hv"][:1] + first["hv"][2:] if water else first["hv"], tag)      # (dMu is 0 in the water, as test 6)
    assert np.isfinite(first["hv"][1]).all() and not np.any(first["hv"][1][~omega]), tag
    r, a, s = o["cmp"]["vHv"]
    G.held(got["vHv"], r, a, tag + " v^T H v")
    G.held(got["vHv"], own, own, tag + " v^T H v against the GPU's own J v")
    # 2. J^T w: device tensors and host memory, all shots and the last alone
    for k in ("jtw", "jtw_host", "jtw_one"):
        for arr in first.get(k, []):
            assert np.isfinite(arr).all() and not np.any(arr[~omega]), (tag, k)
    assert all(np.array_equal(x, y) for x, y in zip(first["jtw"], first["jtw_host"])), (tag, "w, model and outputs in host memory")
    r, a, s = o["cmp"]["<v,JTw>"]
    G.held(got["<v,JTw>"], r, a, tag + " <v, J^T w>", scale=s)
    if "jtw_one" in first:
        r, a, s = o["cmp"]["<v,JTw> one shot"]
        G.held(got["<v,JTw> one shot"], r, a, tag + " <v, J^T w> of shot %d alone" % o["one"], scale=s)
    # 3. the exact gradient
    mis, g = first["exact"][0], first["exact"][1:]
    for arr in g:
        assert np.isfinite(arr).all() and not np.any(arr[~omega]), (tag, "exact gradient")
    assert np.array_equal(mis, first["plain"][0]), (tag, float(mis), float(first["plain"][0]))
    assert all(np.array_equal(x, y) for x, y in zip(first["plain"], first["plain_after"])), (tag, "a plain backward after the exact call")
    assert first["parts"] == first["parts_after"], (tag, first["parts"], first["parts_after"])
    assert "exact adjoint" in first["status"], (tag, first["status"])
    r, a, s = o["cmp"]["<g,d>"]
    dev, yard = abs(got["<g,d>"] - r), abs(a - r)
    print("%s <g, d>: got %.8e, reference %.8e, deviation %.2e (the two oracle builds %.2e, conditioning term %.1e)" % (tag, got["<g,d>"], r, dev / s, yard / s, cond_g))
    assert np.isfinite(got["<g,d>"]) and dev <= (TOL + cond_g) * s + 3.0 * yard, (tag, "<g, d>", dev / s, yard / s, cond_g)
    return True
