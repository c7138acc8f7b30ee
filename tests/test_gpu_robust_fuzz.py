"""Seeded random small problems for the robust misfits (parameter keys robust_misfit / robust_delta / robust_quantile) through every pass
(-m gpu): Session::misfit_chain, gn_chain, Session::born's observed gather for the IRLS weight (obs_->acquire / release_all in
csrc/session_born.cpp), Session::data_misfit / data_gn with the borrowed fourth gather, k_robust_trace and the fixed-order sum of
csrc/robust_misfit.hip where tests/test_gpu_robust_misfit.py, with its one grid, does not reach -- ragged channel counts, a call on ONE
shot of a ragged survey that is not shot 0 (the store's offset for the observed gather of the weight), gauge channels and directional
sensitivities, general (scattered) receivers whose gathers span 30 decades, a water layer, nPad > 0 with dz != dx, every option set of
the Born fuzz, robust_quantile 0.99 and 1.0 beside the default, shots in which some traces are dead (A == 0) beside live ones, and the
empty window.

Every seed is the draw of tests/test_gpu_conditioned_gn_fuzz.py (draw_problem + draw_born + draw_conditioned, unchanged) written once
more under the keys (fuzz_draws.draw_robust, generator default_rng(ROB_SEED0 + seed)): the penalty from (huber, cauchy), robust_delta
from (0.1, 0.5), robust_quantile from (absent: the default 0.9; 0.99; 1.0), the keyed modes "filter", "window", "both", "narrow" that
the seed drew and in one draw of four the keys ALONE (if_win and filter stripped, C the end taper).  The same file without the keys is
the twin of the bit-identity checks.  The observed gathers are the oracle's of lame_true with spikes of 100 x the trace's peak on every
live trace: five on samples above A, chosen on the plain build's C obs inside the window, one where five do not fit (q = 1.0: on the
trace's maximum, A then IS the spike) -- robust_ref.spike_plan / put_spikes say what that does to A.  Where more than half of the call's
traces are dead in the reference (short windows under if_win without a filter: the zeros take rank k) the quantile steps up to the next
of 0.9, 0.99, 1.0; the line of the seed says so.

Reference (fuzz_sides.robust_oracle_side, no GPU; tests/test_robust_fuzz_reference.py runs it on the default seeds): syn, J v, J d of
born_ref and obs of lame_true on both oracle builds; psi, w, A of tests/robust_ref.py in float64 on the float32 gathers; C and C^T each
build's own; gradients of a reference-style pass from oracle.cufd(adj_src=...), through the member survey on gauge draws.  Tolerances are
the existing nominals (1e-3 products and gradients, 1e-4 misfit and gathers, + 3 x the two builds' difference) plus the penalty's
conditioning terms (fuzz_sides.cond_robust derives them) and nothing else:
    a  4 eps |psi'(u) . C syn| / |psi|                            adjoint sources and gradients
    m  4 eps |psi| |C syn| / misfit                               the misfit
    p  4 eps |w'(u) / (delta A) . C syn . C J v| / |w . C J v|    the products
    1  the spiked obs installed for all shots; gauss_newton(exact=True) on v and on d: 0 outside Omega (hvMu exempt under water, as in
       the conditioned fuzz); a second call the same bits; v^T H v against |W^1/2 Z C J v|^2; <d, H v> against <v, H d> and both against
       <W^1/2 Z C J d, W^1/2 Z C J v> on the scale of the two norms; ids = [k] alone (k the last live shot, never shot 0 where two are
       live) against shot k's own value
    2  gauss_newton(exact=False) on v against the oracle's gradient with adj_src = -C^T Z W Z C J v injected, and the reference-style
       backward gradient against the oracle's with a injected (fuzz_common.gradient_miss, water included)
    3  the forward misfit against backward(exact_adjoint=True)'s to 1e-4 and against the reference; the exact gradient 0 outside Omega;
       <g, d> against -<Z C J d, psi> -- on its own scale where cos(Z C J d, psi) >= 0.4, else on |Z C J d| |psi| (the spikes own psi and
       the model difference explains none of them; tests/test_robust_fuzz_reference.py names the seeds)
    4  data_misfit / data_gn(obs=) on the reference's own gathers (obs, syn, J v): device and host pointers the same bits; the misfit; adj
       and out per gather in rel-L2, alt the other build's C on the SAME gathers, with the subnormal exemption of fuzz_held.gathers_held;
       the call ids = [k] on shot k's gathers alone; the reference's dead traces exactly 0 in both outputs under "window" and "alone"
    5  born gathers and born_adjoint with the caller's w: the bits of the twin file without the keys
A draw whose record is not live, whose conditioning term or yardstick exceeds 1e-2, or in which fewer than one live sample in 100 lies
outside the threshold (or inside it) is drawn again with the record two, then four times as long (fuzz_sides.robust_oracle_side); still
so then it is reported as xfail, never passed (no default seed is).  Every deviation is printed before the one assertion at the end.

profiles/r30_robust_fuzz.txt holds the deviations measured on the MI355X and what three deliberately wrong builds of the library do to
these comparisons."""
import numpy as np
import pytest
import torch

import exact_adjoint_ref as X
import fuzz_common as C
import problems as P
import robust_ref as R
from born_ref import GRADS
from exact_adjoint_ref import cuda, outside_is_zero
from fuzz_held import flat, gathers_held, held, unflat
from fuzz_sides import describe_robust, robust_oracle_side

pytestmark = pytest.mark.gpu


def _np(ts):
    return [t.cpu().numpy() for t in ts]


@pytest.mark.parametrize("seed", C.seeds("SEPFWI_ROB_FUZZ"))
def test_random_problem_matches_oracle_robust(tmp_path, oracle, oracle_nvfma, hip_ops, seed):
    """As test_random_problem_matches_oracle_envelope, under the robust keys."""
    from sepfwi import fwi_ops
    o, scale = C.settled(robust_oracle_side, tmp_path, oracle, oracle_nvfma, seed, "the record is not live, a conditioning term exceeds 1e-2 or one branch of the penalty is empty (robust_oracle_side)")
    d, b, r, ref, alt, cr = o["d"], o["b"], o["r"], o["ref"], o["alt"], o["cond"]
    pb, twin, opts, water, k = r["pb"], r["twin"], b["opts"], d["water"], o["one"]
    fn, stf, ids = pb["para_fname"], pb["Stf"], pb["Shot_ids"]
    tag = "robust fuzz seed %d (%s)" % (seed, describe_robust(o, scale))
    fwi_ops.release()
    m, v, dm = cuda(o["m"]), cuda(o["v"]), cuda(o["dm"])
    obs, syn, jv = ref["obs"], ref["syn"], ref["jv"]
    one = slice(k, k + 1)
    with P.kernel_options(**opts):      # every GPU call in one session under the draw's options
        if opts.get("quiet_skip"):      # a plain misfit call with quiet_skip = 1 first: it leaves quiet maps behind in the session
            hip_ops.obscalc(*[t.cuda() for t in pb["lame_true"]], stf, 1, ids, fn)
            hip_ops.forward(*m, stf, 0, ids, fn)
        for i, sid in enumerate(ids.tolist()):      # the weight of the products reads the observed gathers from the store
            hip_ops.set_observed(fn, sid, torch.from_numpy(np.ascontiguousarray(obs[i])))
        hv = _np(hip_ops.gauss_newton(*m, *v, stf, 1, ids, fn, exact=True))
        again = _np(hip_ops.gauss_newton(*m, *v, stf, 1, ids, fn, exact=True))
        hd = _np(hip_ops.gauss_newton(*m, *dm, stf, 1, ids, fn, exact=True))
        hv_one = _np(hip_ops.gauss_newton(*m, *v, stf, 1, ids[one], fn, exact=True)) if len(jv) > 1 else None
        hv_ref = _np(hip_ops.gauss_newton(*m, *v, stf, 1, ids, fn, exact=False))
        f0 = float(hip_ops.forward(*m, stf, 0, ids, fn)[0])
        ex = hip_ops.backward(*m, stf, 1, ids, fn, exact_adjoint=True)
        f, g = float(ex[0]), _np(ex[1:4])
        g_ref = _np(hip_ops.backward(*m, stf, 1, ids, fn)[1:4])
        fd, ad = hip_ops.data_misfit(flat(obs).cuda(), flat(syn).cuda(), ids, fn)
        fh, ah = hip_ops.data_misfit(flat(obs), flat(syn), ids, fn)
        gd = hip_ops.data_gn(flat(syn).cuda(), flat(jv).cuda(), ids, fn, obs=flat(obs).cuda())
        gh = hip_ops.data_gn(flat(syn), flat(jv), ids, fn, obs=flat(obs))
        f1, a1 = hip_ops.data_misfit(flat(obs[one]).cuda(), flat(syn[one]).cuda(), ids[one], fn)
        g1 = hip_ops.data_gn(flat(syn[one]).cuda(), flat(jv[one]).cuda(), ids[one], fn, obs=flat(obs[one]).cuda())
        born = [[x["ett"].cpu() for x in hip_ops.born(*m, *v, stf, 1, ids, p)] for p in (fn, twin["para_fname"])]
        w = [{"ett": torch.from_numpy(np.ascontiguousarray(x))} for x in ref["jd"]]
        jtw = [hip_ops.born_adjoint(*m, w, stf, 1, ids, p) for p in (fn, twin["para_fname"])]
    fwi_ops.release()

    omega = X.mask_omega(pb)
    got = {"vHv": X.model_dot(o["v"], hv), "<d,Hv>": X.model_dot(o["dm"], hv), "<v,Hd>": X.model_dot(o["v"], hd), "misfit": f,
           "<g,d>": X.model_dot(o["dm"], g)}
    if hv_one is not None:
        got["vHv one shot"] = X.model_dot(o["v"], hv_one)
    line = {key: "%.2e (builds %.2e)" % (abs(got[key] - x) / max(s, 1e-300), o["yard"][key]) for key, (x, a, s) in o["cmp"].items()}
    line.update({"cond a / m / p": "%.1e / %.1e / %.1e" % (cr["a"], cr["m"], cr["p"]), "the one shot": "%d of %d" % (k, len(jv)),
                 "cos(ZCJd, psi)": "%.3f" % ref["cos_dr"], "A between the builds": "%.1e" % o["yard"]["A"], "dead share": "%.3f" % o["dead_share"],
                 "peak |syn|": "%.1e" % max(float(np.abs(s).max()) for s in syn)})
    print("%s: %r" % (tag, line))
    if not o["target"]:
        pytest.xfail("seed %d: no target -- the two oracle builds differ by %r of the scales (cond %r)" % (seed, o["yard"], cr))

    # every deviation is printed before anything is asserted: a miss goes to `bad`, the one assertion is at the end
    bad = []
    check = lambda ok, what: None if ok else bad.append(what)
    # 1. the exact product
    check(all(np.array_equal(x, y) for x, y in zip(hv, again)), "the second call of the session")
    for what, arrs in (("H v", hv), ("H d", hd), ("H_k v", hv_one or [])):
        outside_is_zero(pb, arrs[:1] + arrs[2:] if water else arrs, (tag, what))      # (as tests/test_gpu_conditioned_gn_fuzz.py)
        assert not arrs or (np.isfinite(arrs[1]).all() and not np.any(arrs[1][~omega])), (tag, what, "hvMu")
    x, a, s = o["cmp"]["vHv"]
    held(bad, got["vHv"], x, a, tag + " v^T H v against |W^1/2 Z C J v|^2", C.GRAD_TOL, cr["p"], name="cond p")
    x, a, s = o["cmp"]["<d,Hv>"]
    held(bad, got["<d,Hv>"], got["<v,Hd>"], got["<v,Hd>"] + (a - x), tag + " symmetry <d, H v> against <v, H d>", C.GRAD_TOL, cr["p"], s, name="cond p")
    held(bad, got["<d,Hv>"], x, a, tag + " <d, H v> against the reference's cross term", C.GRAD_TOL, cr["p"], s, name="cond p")
    held(bad, got["<v,Hd>"], x, a, tag + " <v, H d> against the reference's cross term", C.GRAD_TOL, cr["p"], s, name="cond p")
    if hv_one is not None:
        x, a, s = o["cmp"]["vHv one shot"]
        held(bad, got["vHv one shot"], x, a, tag + " v^T H_k v of shot %d alone" % k, C.GRAD_TOL, cr["p"], name="cond p")
    # 2. the reference-style product and gradient
    for what, arrs, sides, cond in (("product", hv_ref, o["gn"], cr["p"]), ("gradient", g_ref, o["grad"], cr["a"])):
        for i, name in enumerate(GRADS):
            rg, ag = sides[0][name], sides[1][name]
            print("%s reference-style %s %s: deviation from the oracle's pass with the adjoint source injected %.2e (the two oracle builds %.2e, cond %.1e)"
                  % (tag, what, name, C.rel(C.d64(arrs[i], rg), rg), C.rel(C.d64(ag, rg), rg), cond))
            miss = C.gradient_miss(arrs[i], rg, ag, C.GRAD_TOL, cond, water)
            check(np.isfinite(arrs[i]).all() and C.l2(rg) > 0 and not miss, "reference-style %s %s: %s" % (what, name, miss))
    # 3. the misfit and the exact gradient
    x, a, s = o["cmp"]["misfit"]
    print("%s: misfit of the exact pass %.8e, of a forward call %.8e (relative gap %.2e), of the reference %.8e (%.2e; the two builds %.2e, cond m %.1e)"
          % (tag, f, f0, abs(f - f0) / f0, x, abs(f - x) / x, abs(a - x) / x, cr["m"]))
    check(abs(f - f0) <= C.MISFIT_TOL * f0, "misfit of the two calls")
    check(C.scalar_held(f, x, a, C.MISFIT_TOL, cond=cr["m"]) and C.scalar_held(f0, x, a, C.MISFIT_TOL, cond=cr["m"]), "misfit")
    check(all(np.isfinite(arr).all() and not np.any(arr[~omega]) for arr in g), "exact gradient outside Omega")
    x, a, s = o["cmp"]["<g,d>"]
    held(bad, got["<g,d>"], x, a, tag + " <g, d> against -<Z C J d, psi>", C.GRAD_TOL, cr["a"], s, name="cond a")
    # 4. the data-space entry points on the reference's own gathers; alt: the other build's C (and C^T) on the same gathers
    check(ad.is_cuda and not ah.is_cuda and fd == fh and torch.equal(ad.cpu(), ah), "data_misfit: host and device pointers differ")
    check(gd.is_cuda and not gh.is_cuda and torch.equal(gd.cpu(), gh), "data_gn: host and device pointers differ")
    f_alt, a_alt, _ = R.data_misfit(oracle_nvfma, pb, obs, syn)
    g_alt = R.data_gn(oracle_nvfma, pb, obs, syn, jv)
    x = ref["misfit"]
    print("%s data_misfit: %.8e, reference %.8e (relative gap %.2e; the other build's C %.2e)" % (tag, fd, x, abs(fd - x) / x, abs(f_alt - x) / x))
    check(C.scalar_held(fd, x, f_alt, C.MISFIT_TOL, cond=cr["m"]), "data_misfit")
    adj, out = unflat(ah, obs), unflat(gh, jv)
    gathers_held(bad, adj, ref["adj"], a_alt, tag + " data_misfit adj", cr["a"], name="cond a")
    gathers_held(bad, out, ref["gn_v"], g_alt, tag + " data_gn", cr["p"], name="cond p")
    gathers_held(bad, unflat(a1, obs[one]), ref["adj"][one], a_alt[one], tag + " data_misfit adj of shot %d alone" % k, cr["a"], name="cond a")
    gathers_held(bad, unflat(g1, jv[one]), ref["gn_v"][one], g_alt[one], tag + " data_gn of shot %d alone" % k, cr["p"], name="cond p")
    check(C.l2(ref["adj"][k]) > 0 and C.l2(ref["gn_v"][k]) > 0, "the reference's own adjoint source of shot %d" % k)
    x1 = ref["misfit_one"]
    c_alt = lambda gs: [R.C_of(oracle_nvfma, pb, gs[k], int(ids[k]))]
    a1_ = R.conditioned_misfit(pb, c_alt(obs), c_alt(syn))[0]
    print("%s data_misfit of shot %d alone: %.8e, reference %.8e (relative gap %.2e)" % (tag, k, f1, x1, abs(f1 - x1) / max(x1, 1e-300)))
    check(C.scalar_held(f1, x1, a1_, C.MISFIT_TOL, cond=cr["m"]), "data_misfit of one shot")
    if r["mode"] in ("window", "alone"):      # no filter: a dead trace is dead for every build, and its rows are 0, not small
        dead = [A == 0.0 for A in ref["A"]]
        print("%s: dead traces per shot %r" % (tag, [int(x.sum()) for x in dead]))
        check(all(not np.any(x[z]) and not np.any(y[z]) for x, y, z in zip(adj, out, dead)), "a dead trace's rows of adj or out are not 0")
    # 5. born and born_adjoint stay in raw data space: the bits of the twin file without the keys
    check(born[0][k].abs().max() > 0 and all(torch.equal(x, y) for x, y in zip(*born)), "born under the keys")
    check(all(t.abs().max() > 0 for t in jtw[0]) and all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(*jtw)), "born_adjoint under the keys")
    assert not bad, (tag, [what.replace(tag, "").strip() for what in bad])
