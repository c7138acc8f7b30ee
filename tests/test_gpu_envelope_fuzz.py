"""Seeded random small problems for the envelope misfit (parameter key if_envelope_misfit) through every pass (-m gpu):
Session::record_background, adjoint_source_conditioned / gn_chain with the third scratch gather, Session::data_misfit / data_gn,
Conditioner::hilbert and the envelope kernels of csrc/conditioning.hip where tests/test_gpu_envelope_misfit.py, with its one geometry,
does not reach -- gauge channels and directional sensitivities in the BACKGROUND gather, ragged channel counts (one born_bg_ reused shot
after shot, an FFT plan per trace count within one call), a call on ONE shot of a ragged survey that is not shot 0 (the window table's
offset for the third gather), a water layer, nPad > 0 with dz != dx, scattered channels whose gathers span 30 decades, gathers that
peak at 4e1 ... 2e4 (the kernels are float32 of the data's third power), and every option set of the Born fuzz.

Every seed is the draw of tests/test_gpu_conditioned_gn_fuzz.py (draw_problem + draw_born + draw_conditioned, unchanged) written once
more with the key added (fuzz_draws.draw_envelope, generator default_rng(ENV_SEED0 + seed)): the keyed modes "filter", "window", "both",
"narrow" that the seed drew, and in one draw of four the key ALONE (if_win and filter stripped, C the end taper).  The same file
without the key is the twin of the bit-identity checks.

Reference (fuzz_sides.envelope_oracle_side, no GPU; tests/test_envelope_fuzz_reference.py runs it on the default seeds): syn, J v, J d
of born_ref and obs of lame_true on both oracle builds; H, e, D, D^T of tests/envelope_ref.py in float64 on the float32 gathers; C and
C^T each build's own; gradients of a reference-style pass from oracle.cufd(adj_src=...), through the member survey on gauge draws.
Tolerances are the existing nominals (1e-3 products and gradients, 1e-4 misfit and gathers, + 3 x the two builds' difference) plus the
envelope's conditioning term and nothing else:
    cond_env = 4 eps (1 + 2 sqrt(E_e / m)),  E_e = 1/2 |e(C syn)|^2, m the misfit                (fuzz_sides.cond_env)
added to the nominal tolerance of gradient-like quantities, twice it to the misfit's.
    1  gauss_newton(exact=True) on v and on d: 0 outside Omega (hvMu exempt under water, as in the conditioned fuzz); a second call the
       same bits; v^T H v against |Z D C J v|^2; <d, H v> against <v, H d> and both against <Z D C J d, Z D C J v> on the scale
       |Z D C J v| |Z D C J d|; ids = [k] alone (k the last live shot, never shot 0 where two are live) against shot k's own |Z D C J v|^2
    2  gauss_newton(exact=False) on v against the oracle's gradient with adj_src = -C^T D^T Z D C J v injected (fuzz_common.gradient_miss)
    3  raw obs installed: the forward misfit against backward(exact_adjoint=True)'s to 1e-4 and against the reference; <g, d> against
       -<Z D C J d, rho>; the reference-style backward gradients against the oracle's gradient with a injected
    4  data_misfit / data_gn on the reference's own gathers (obs, syn, J v): device and host pointers the same bits; the misfit; adj and
       out per gather in rel-L2 (the channels span 30 decades: not element by element), bound (1e-4 + cond_env) |ref| + 3 |alt - ref| with
       alt the other build's C on the SAME gathers; the call ids = [k] on shot k's gathers alone
    5  born gathers and born_adjoint with the caller's w: the bits of the twin file without the key
A draw that conditioned_oracle_side would draw again, whose cond_env exceeds 1e-2 or one of whose yardsticks exceeds 1e-2 of its scale
(fuzz_sides.envelope_oracle_side says which, and on which seeds) is drawn again with the record two, then four times as long; still so
then it is reported as xfail, never passed (no default seed is).  Every deviation is printed before the one assertion at the end.

What the draws found (profiles/r23_envelope_fuzz.txt, with the deviations measured on the MI355X and what deliberately wrong builds do
to them): k_env_residual formed rho as e(o) - e(s) in float32, off by eps |e(s)|; where a channel's data nearly fit (|rho| / |e(s)| 1e-4
on shot 0 of seed 0, 1.6e-7 on shot 3 of seed 10) the adjoint source of data_misfit was 4.9e-3 resp. 1.4 off the reference in rel-L2
(comparison 4).  The kernel now forms rho from the data residual, d (o + s) + (H d)(H d + 2 H s) with d = o - s."""
import numpy as np
import pytest
import torch

import cond_gn_ref as G
import envelope_ref as E
import exact_adjoint_ref as X
import fuzz_common as C
import problems as P
from born_ref import GRADS
from exact_adjoint_ref import cuda, outside_is_zero
from fuzz_held import flat, gathers_held, held, unflat
from fuzz_sides import describe_envelope, envelope_oracle_side

pytestmark = pytest.mark.gpu


def _np(ts):
    return [t.cpu().numpy() for t in ts]


@pytest.mark.parametrize("seed", C.seeds("SEPFWI_ENV_FUZZ"))
def test_random_problem_matches_oracle_envelope(tmp_path, oracle, oracle_nvfma, hip_ops, seed):
    """As test_random_problem_matches_oracle_conditioned, under the key."""
    from sepfwi import fwi_ops
    o, scale = C.settled(envelope_oracle_side, tmp_path, oracle, oracle_nvfma, seed, "the record is not live, the inputs do not discriminate or cond_env > 1e-2 (envelope_oracle_side)")
    d, b, e, ref, alt, ce = o["d"], o["b"], o["e"], o["ref"], o["alt"], o["cond_env"]
    pb, twin, opts, water, k = e["pb"], e["twin"], b["opts"], d["water"], o["one"]
    fn, stf, ids = pb["para_fname"], pb["Stf"], pb["Shot_ids"]
    tag = "envelope fuzz seed %d (%s)" % (seed, describe_envelope(o, scale))
    fwi_ops.release()
    m, v, dm = cuda(o["m"]), cuda(o["v"]), cuda(o["dm"])
    obs, syn, jv = ref["obs"], ref["syn"], ref["jv"]
    one = slice(k, k + 1)
    with P.kernel_options(**opts):      # every GPU call in one session under the draw's options
        if opts.get("quiet_skip"):      # a plain misfit call with quiet_skip = 1 first: it leaves quiet maps behind in the session
            hip_ops.obscalc(*[t.cuda() for t in pb["lame_true"]], stf, 1, ids, fn)
            hip_ops.forward(*m, stf, 0, ids, fn)
        hv = _np(hip_ops.gauss_newton(*m, *v, stf, 1, ids, fn, exact=True))
        again = _np(hip_ops.gauss_newton(*m, *v, stf, 1, ids, fn, exact=True))
        hd = _np(hip_ops.gauss_newton(*m, *dm, stf, 1, ids, fn, exact=True))
        hv_one = _np(hip_ops.gauss_newton(*m, *v, stf, 1, ids[one], fn, exact=True)) if len(jv) > 1 else None
        hv_ref = _np(hip_ops.gauss_newton(*m, *v, stf, 1, ids, fn, exact=False))
        for i, sid in enumerate(ids.tolist()):
            hip_ops.set_observed(fn, sid, torch.from_numpy(np.ascontiguousarray(obs[i])))
        f0 = float(hip_ops.forward(*m, stf, 0, ids, fn)[0])
        ex = hip_ops.backward(*m, stf, 1, ids, fn, exact_adjoint=True)
        f, g = float(ex[0]), _np(ex[1:4])
        g_ref = _np(hip_ops.backward(*m, stf, 1, ids, fn)[1:4])
        fd, ad = hip_ops.data_misfit(flat(obs).cuda(), flat(syn).cuda(), ids, fn)
        fh, ah = hip_ops.data_misfit(flat(obs), flat(syn), ids, fn)
        gd = hip_ops.data_gn(flat(syn).cuda(), flat(jv).cuda(), ids, fn)
        gh = hip_ops.data_gn(flat(syn), flat(jv), ids, fn)
        f1, a1 = hip_ops.data_misfit(flat(obs[one]).cuda(), flat(syn[one]).cuda(), ids[one], fn)
        g1 = hip_ops.data_gn(flat(syn[one]).cuda(), flat(jv[one]).cuda(), ids[one], fn)
        born = [[x["ett"].cpu() for x in hip_ops.born(*m, *v, stf, 1, ids, p)] for p in (fn, twin["para_fname"])]
        w = [{"ett": torch.from_numpy(np.ascontiguousarray(x))} for x in ref["jd"]]
        jtw = [hip_ops.born_adjoint(*m, w, stf, 1, ids, p) for p in (fn, twin["para_fname"])]
    fwi_ops.release()

    omega = X.mask_omega(pb)
    got = {"vHv": X.model_dot(o["v"], hv), "<d,Hv>": X.model_dot(o["dm"], hv), "<v,Hd>": X.model_dot(o["v"], hd), "misfit": f,
           "<g,d>": X.model_dot(o["dm"], g)}
    if hv_one is not None:
        got["vHv one shot"] = X.model_dot(o["v"], hv_one)
    line = {key: "%.2e (builds %.2e)" % (abs(got[key] - r) / max(s, 1e-300), o["yard"][key]) for key, (r, a, s) in o["cmp"].items()}
    line.update({"cond_env": "%.1e" % ce, "the one shot": "%d of %d" % (k, len(jv)), "cos(ZDCJd, rho)": "%.3f" % ref["cos_dr"],
                 "peak |syn|": "%.1e" % max(float(np.abs(s).max()) for s in syn)})
    print("%s: %r" % (tag, line))
    if not o["target"]:
        pytest.xfail("seed %d: no target -- the two oracle builds differ by %r of the scales (cond_env %.1e)" % (seed, o["yard"], ce))

    # every deviation is printed before anything is asserted: a miss goes to `bad`, the one assertion is at the end
    bad = []
    check = lambda ok, what: None if ok else bad.append(what)
    # 1. the exact product
    check(all(np.array_equal(x, y) for x, y in zip(hv, again)), "the second call of the session")
    for what, arrs in (("H v", hv), ("H d", hd), ("H_k v", hv_one or [])):
        outside_is_zero(pb, arrs[:1] + arrs[2:] if water else arrs, (tag, what))      # (as tests/test_gpu_conditioned_gn_fuzz.py)
        assert not arrs or (np.isfinite(arrs[1]).all() and not np.any(arrs[1][~omega])), (tag, what, "hvMu")
    r, a, s = o["cmp"]["vHv"]
    held(bad, got["vHv"], r, a, tag + " v^T H v against |Z D C J v|^2", C.GRAD_TOL, ce)
    r, a, s = o["cmp"]["<d,Hv>"]
    held(bad, got["<d,Hv>"], got["<v,Hd>"], got["<v,Hd>"] + (a - r), tag + " symmetry <d, H v> against <v, H d>", C.GRAD_TOL, ce, s)
    held(bad, got["<d,Hv>"], r, a, tag + " <d, H v> against <Z D C J d, Z D C J v>", C.GRAD_TOL, ce, s)
    held(bad, got["<v,Hd>"], r, a, tag + " <v, H d> against <Z D C J d, Z D C J v>", C.GRAD_TOL, ce, s)
    if hv_one is not None:
        r, a, s = o["cmp"]["vHv one shot"]
        held(bad, got["vHv one shot"], r, a, tag + " v^T H_k v of shot %d alone" % k, C.GRAD_TOL, ce)
    # 2. the reference-style product, 3. the reference-style gradient
    for what, arrs, sides in (("product", hv_ref, o["gn"]), ("gradient", g_ref, o["grad"])):
        for i, name in enumerate(GRADS):
            rg, ag = sides[0][name], sides[1][name]
            print("%s reference-style %s %s: deviation from the oracle's pass with the adjoint source injected %.2e (the two oracle builds %.2e, cond_env %.1e)"
                  % (tag, what, name, C.rel(C.d64(arrs[i], rg), rg), C.rel(C.d64(ag, rg), rg), ce))
            miss = C.gradient_miss(arrs[i], rg, ag, C.GRAD_TOL, ce, water)
            check(np.isfinite(arrs[i]).all() and C.l2(rg) > 0 and not miss, "reference-style %s %s: %s" % (what, name, miss))
    # 3. the misfit and the exact gradient
    r, a, s = o["cmp"]["misfit"]
    print("%s: misfit of the exact pass %.8e, of a forward call %.8e (relative gap %.2e), of the reference %.8e (%.2e; the two builds %.2e, 2 cond_env %.1e)"
          % (tag, f, f0, abs(f - f0) / f0, r, abs(f - r) / r, abs(a - r) / r, 2.0 * ce))
    check(abs(f - f0) <= C.MISFIT_TOL * f0, "misfit of the two calls")
    check(C.scalar_held(f, r, a, C.MISFIT_TOL, cond=2.0 * ce) and C.scalar_held(f0, r, a, C.MISFIT_TOL, cond=2.0 * ce), "misfit")
    check(all(np.isfinite(arr).all() and not np.any(arr[~omega]) for arr in g), "exact gradient outside Omega")
    r, a, s = o["cmp"]["<g,d>"]
    held(bad, got["<g,d>"], r, a, tag + " <g, d> against -<Z D C J d, rho>", C.GRAD_TOL, ce, s)
    # 4. the data-space entry points on the reference's own gathers; alt: the other build's C (and C^T) on the same gathers
    check(ad.is_cuda and not ah.is_cuda and fd == fh and torch.equal(ad.cpu(), ah), "data_misfit: host and device pointers differ")
    check(gd.is_cuda and not gh.is_cuda and torch.equal(gd.cpu(), gh), "data_gn: host and device pointers differ")
    f_alt, a_alt, _, _ = E.data_misfit(oracle_nvfma, pb, obs, syn)
    g_alt = E.data_gn(oracle_nvfma, pb, syn, jv)
    r = ref["misfit"]
    print("%s data_misfit: %.8e, reference %.8e (relative gap %.2e; the other build's C %.2e)" % (tag, fd, r, abs(fd - r) / r, abs(f_alt - r) / r))
    check(C.scalar_held(fd, r, f_alt, C.MISFIT_TOL, cond=2.0 * ce), "data_misfit")
    gathers_held(bad, unflat(ah, obs), ref["adj"], a_alt, tag + " data_misfit adj", ce)
    gathers_held(bad, unflat(gh, jv), ref["gn_v"], g_alt, tag + " data_gn", ce)
    gathers_held(bad, unflat(a1, obs[one]), ref["adj"][one], a_alt[one], tag + " data_misfit adj of shot %d alone" % k, ce)
    gathers_held(bad, unflat(g1, jv[one]), ref["gn_v"][one], g_alt[one], tag + " data_gn of shot %d alone" % k, ce)
    check(C.l2(ref["adj"][k]) > 0 and C.l2(ref["gn_v"][k]) > 0, "the reference's own adjoint source of shot %d" % k)
    r1 = 0.5 * float((ref["rho"][k] ** 2).sum())
    a1_ = 0.5 * float((E.rho(E.C_of(oracle_nvfma, pb, obs[k], ids[k]), E.C_of(oracle_nvfma, pb, syn[k], ids[k])) ** 2).sum())
    print("%s data_misfit of shot %d alone: %.8e, reference %.8e (relative gap %.2e)" % (tag, k, f1, r1, abs(f1 - r1) / max(r1, 1e-300)))
    check(C.scalar_held(f1, r1, a1_, C.MISFIT_TOL, cond=2.0 * ce), "data_misfit of one shot")
    # 5. born and born_adjoint stay in raw data space: the bits of the twin file without the key
    check(born[0][k].abs().max() > 0 and all(torch.equal(x, y) for x, y in zip(*born)), "born under the key")
    check(all(t.abs().max() > 0 for t in jtw[0]) and all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(*jtw)), "born_adjoint under the key")
    assert not bad, (tag, bad)
