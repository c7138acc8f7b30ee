"""Seeded random small problems for the exact discrete adjoint: HIP (csrc/exact_adjoint.hip, csrc/session_exact.cpp, sepfwi_adjoint_exact)
against J itself outside the GPU (-m gpu).  tests/test_gpu_exact_adjoint.py holds the pass on hand-picked problems; this file holds it
where those do not reach: channels INSIDE the absorbing layers (the order of injection and k_exact_b, the priming of Q for column
nSteps-1), the column where the x strips of S and V differ, ragged channel counts with the caller's w, w in host memory, the exact
gradient of a joint / gauge / ragged misfit (k_geo_residual), padded widths below 64, layer widths 4 ... 12, nPad 0 ... 8 with dz != dx,
a water layer, and a session whose earlier call left quiet maps behind.

Every seed is a draw of tests/test_gpu_fuzz.py (fuzz_draws.draw_problem) changed by tests/test_gpu_born_fuzz.py (draw_born: conditioning
keys removed, option set, ragged counts, joint weights, gauge G 2 ... 5) and then by fuzz_draws.draw_exact from a generator of its own
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

Reference (fuzz_sides.exact_oracle_side, no GPU; tests/test_exact_adjoint_fuzz_reference.py runs it on the default seeds): per oracle build
three runs of tests/born_ref.py through born_ref.born_side -- (m_init, v): syn and J v; (m_init, d): J d; (m_true, 0): obs -- and
r = obs - syn in float64, obs rounded to float32 as it is installed.  All dot products in float64.  Tolerances are those of
tests/test_gpu_exact_adjoint.py (exact_adjoint_ref.held, TOL = 1e-3, 3 x the difference of the same quantity between the two oracle builds), none new:
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
the wave has not come back from where the models differ -- is drawn again with the record two, then four times as long (exact_oracle_side);
still not live then, it is an xfail too.
profiles/r12_exact_adjoint_fuzz.txt holds the deviations measured on the MI355X and what the fuzz does to five deliberately wrong
variants of the pass."""
import numpy as np
import pytest
import torch

import exact_adjoint_ref as X
import fuzz_common as C
import problems as P
from born_ref import COMPS
from exact_adjoint_ref import TOL, capi, cuda, held, outside_is_zero
from fuzz_sides import describe_exact, exact_oracle_side, wdot

pytestmark = pytest.mark.gpu


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
    m, v = cuda(o["m"]), cuda(o["v"])
    out = {}
    out["hv"] = _np(hip_ops.gauss_newton(*m, *v, stf, 1, ids, fn, exact=True))
    out["own"] = [{c: g[c].cpu().numpy() for c in COMPS} for g in hip_ops.born(*m, *v, stf, 1, ids, fn, components=COMPS)]
    w = [{c: torch.from_numpy(a).cuda() for c, a in sh.items()} for sh in ref["w"]]
    out["jtw"] = _np(hip_ops.born_adjoint(*m, w, stf, 1, ids, fn))
    rc, out["jtw_host"] = capi(pb, fn, [np.ascontiguousarray(a, dtype=np.float32) for a in o["m"]], w=flat_w(ref), host_out=True)
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


@pytest.mark.parametrize("seed", C.seeds("SEPFWI_EXACT_FUZZ"))
def test_random_problem_matches_oracle_exact_adjoint(tmp_path, oracle, oracle_nvfma, hip_ops, seed):
    """As test_random_problem_matches_oracle, with its re-draw of a record that ends before the wave reaches the channels."""
    from sepfwi import fwi_ops
    o, scale = C.settled(exact_oracle_side, tmp_path, oracle, oracle_nvfma, seed, "the record is not live (exact_oracle_side)")
    d, b, ref, alt = o["d"], o["b"], o["ref"], o["alt"]
    pb, opts, water = d["pb"], b["opts"], d["water"]
    fn = pb["para_fname"]
    tag = "exact fuzz seed %d (%s)" % (seed, describe_exact(o, scale))
    weights = b["weights"] or (1.0, 0.0, 0.0)
    omega = X.mask_omega(pb)
    fwi_ops.release()
    with P.kernel_options(**opts):      # 4. every GPU call under the draw's options
        if opts.get("quiet_skip"):
            # a plain misfit call with quiet_skip = 1 first: it leaves quiet maps behind in the session that then serves the exact pass
            hip_ops.obscalc(*[t.cuda() for t in pb["lame_true"]], pb["Stf"], 1, pb["Shot_ids"], fn)
            hip_ops.forward(*cuda(o["m"]), pb["Stf"], 0, pb["Shot_ids"], fn)
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
    outside_is_zero(pb, first["hv"][:1] + first["hv"][2:] if water else first["hv"], tag)      # (dMu is 0 in the water, as test 6)
    assert np.isfinite(first["hv"][1]).all() and not np.any(first["hv"][1][~omega]), tag
    r, a, s = o["cmp"]["vHv"]
    held(got["vHv"], r, a, tag + " v^T H v")
    held(got["vHv"], own, own, tag + " v^T H v against the GPU's own J v")
    # 2. J^T w: device tensors and host memory, all shots and the last alone
    for k in ("jtw", "jtw_host", "jtw_one"):
        for arr in first.get(k, []):
            assert np.isfinite(arr).all() and not np.any(arr[~omega]), (tag, k)
    assert all(np.array_equal(x, y) for x, y in zip(first["jtw"], first["jtw_host"])), (tag, "w, model and outputs in host memory")
    r, a, s = o["cmp"]["<v,JTw>"]
    held(got["<v,JTw>"], r, a, tag + " <v, J^T w>", scale=s)
    if "jtw_one" in first:
        r, a, s = o["cmp"]["<v,JTw> one shot"]
        held(got["<v,JTw> one shot"], r, a, tag + " <v, J^T w> of shot %d alone" % o["one"], scale=s)
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
    assert C.scalar_held(got["<g,d>"], r, a, TOL, s, cond_g), (tag, "<g, d>", dev / s, yard / s, cond_g)
