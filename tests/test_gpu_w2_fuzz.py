"""Seeded random small problems for the W2 misfit (parameter keys if_w2_misfit / w2_beta) through every pass (-m gpu): the if_w2_misfit
branch of Session::misfit_chain and csrc/w2_misfit.hip where tests/test_gpu_w2_misfit.py, with its one grid, does not reach -- w2_beta
0.5, 8 and 16 beside the default, ragged channel counts, a call on ONE shot of a ragged survey that is not shot 0, gauge channels and
directional sensitivities, general (scattered) receivers whose gathers span tens of decades, a water layer, nPad > 0 with dz != dx, the
option sets of the Born fuzz (the default seeds draw eight of the ten), shots in which a trace is dead (A == 0) beside live ones, and the
empty window.

Every seed is the draw of tests/test_gpu_conditioned_gn_fuzz.py (draw_problem + draw_born + draw_conditioned, unchanged) written once
more under the key (fuzz_draws.draw_w2, generator default_rng(W2_SEED0 + seed)): w2_beta from (absent: the default 3; 0.5; 8; 16), the
keyed modes "filter", "window", "both", "narrow" that the seed drew and in one draw of four the key ALONE (if_win and filter stripped,
C the end taper).  The same file without the two keys is the twin of the bit-identity checks.  The observed gathers are the oracle's of
lame_true; in one draw of two ONE channel of the one-shot call's shot is silenced (exact zeros: the conditioned draw has no dead trace
of its own).

CHAIN OF CUSTODY.  The map from the gathers to the adjoint source amplifies a rounding of its input (tests/test_w2_reference.py), and
its derivative jumps where F_i crosses a node G_j: there c_i changes by the factor g_j / g_(j+1).  So the adjoint source is never
re-derived from one side's gathers and compared with the other side's, and no first-order conditioning term stands in for that.  Every
comparison is on IDENTICAL float32 inputs, or linear in an adjoint source that both sides share.  The library's own raw synthetic
gathers come from obscalc of lame_init under the same option set, into a second directory with the conditioning and W2 keys stripped;
a_lib, f_lib = data_misfit(obs, own syn) on the whole call and on shot k alone (k the last live shot, never shot 0 where two are live).
    1  a_lib is right: w2_held.on_identical_inputs on (obs, own syn), 8 EPS on the misfit, 8 EPS per trace on the window sets, 16 EPS
       rel-L2 under filter; the one-shot call the bits of the full call's rows of shot k; the one-shot misfits of all shots sum to the
       full one within 4 EPS (float32 roundings of sums formed in double); the reference's dead traces exactly 0 under "window", "alone"
    2  the passes use that misfit: f of forward (calc_id 0), of backward and of backward(exact_adjoint=True) against f_lib to
       (8 + 2 kappa_W) EPS f_lib -- the 8 EPS of tests/test_gpu_w2_misfit.py plus what a one-rounding difference between obscalc's
       gathers and the call's own would do by the reference's measure (w2_ref.amplification, random signs: the factor 2)
    3  the reference-style gradient, the whole call and ids = [k], against the oracle's backward pass with adj_src = a_lib injected, on
       both builds, through the member survey on gauge draws: fuzz_common.gradient_miss at GRAD_TOL with 3 x the two builds'
       difference, water included.  Linear in a_lib: no W2 conditioning enters it
    4  the exact gradient: 0 outside Omega; against -J^T a_lib of born_adjoint (the w mode) in rel-L2 to (16 + 2 kappa_a) EPS (the
       1e-5 of tests/test_gpu_w2_misfit.py::test_exact_gradient with the draw's own amplification in the place of 1e2); <g, v> and
       <g, d> against -<a_lib, J v> and -<a_lib, J d>, J of tests/born_ref.py on both builds, to exact_adjoint_ref.held's tolerances
       (on their own scale where the cosine is at least 0.4, else on |a_lib| |J v|); a second call the same bits
    5  the rest: born and born_adjoint under the keys the bits of the twin file; gauss_newton (both modes) and data_gn refused with
       code -1 and the key's name; a gradient call on the twin before and after the keyed calls the same bits and launch count
A draw whose record is not live, whose build yardstick exceeds the cap or whose kappa_a exceeds 1e3 is drawn again with the record two,
then four times as long (fuzz_sides.w2_oracle_side); still so then it is reported as xfail, never passed (no default seed is:
tests/test_w2_fuzz_reference.py).  Every deviation is printed before the one assertion at the end.

profiles/r31_w2_fuzz.txt holds the deviations measured on the MI355X and what three deliberately wrong builds of the library do to
these comparisons."""
import numpy as np
import pytest
import torch

import cond_gn_ref as G
import exact_adjoint_ref as X
import fuzz_common as C
import problems as P
import w2_held as H
import w2_ref as W
from born_ref import GRADS
from exact_adjoint_ref import cuda
from fuzz_held import flat, held
from fuzz_sides import W2_KAPPA_CAP, describe_w2, plain_of_w2, w2_gradients, w2_oracle_side

pytestmark = pytest.mark.gpu
EPS = H.EPS
COS = 0.4      # <g, v> on its own scale where cos(a_lib, J v) is at least this, else on the product of the norms


def _np(ts):
    return [t.cpu().numpy() for t in ts]


@pytest.mark.parametrize("seed", C.seeds("SEPFWI_W2_FUZZ"))
def test_random_problem_matches_oracle_w2(tmp_path, oracle, oracle_nvfma, hip_ops, seed):
    """As test_random_problem_matches_oracle_robust, under the W2 keys and by chain of custody (module docstring)."""
    from sepfwi import _native, fwi_ops
    from sepfwi import utils as ft
    o, scale = C.settled(w2_oracle_side, tmp_path, oracle, oracle_nvfma, seed, "the record is not live, a build yardstick exceeds 1e-2 or kappa_a exceeds 1e3 (w2_oracle_side)")
    d, b, w, ref, alt = o["d"], o["b"], o["w"], o["ref"], o["alt"]
    pb, twin, opts, water, k = w["pb"], w["twin"], b["opts"], d["water"], o["one"]
    fn, tfn, stf, ids = pb["para_fname"], twin["para_fname"], pb["Stf"], pb["Shot_ids"]
    tag = "w2 fuzz seed %d (%s)" % (seed, describe_w2(o, scale))
    fwi_ops.release()
    m, v = cuda(o["m"]), cuda(o["v"])
    obs, one = ref["obs"], slice(k, k + 1)
    bad = []
    check = lambda ok, what: None if ok else bad.append(what)

    def identical(syn_, what, **kw):      # w2_held.on_identical_inputs prints, then asserts: a miss goes to `bad` like every other
        try:
            return H.on_identical_inputs(oracle, hip_ops, pb, kw.pop("obs", obs), syn_, what, **kw)
        except AssertionError as e:
            bad.append("%s: %s" % (what, str(e)[:300]))
            return None

    with P.kernel_options(**opts):      # every GPU call in one session under the draw's options
        if opts.get("quiet_skip"):      # a plain misfit call with quiet_skip = 1 first: it leaves quiet maps behind in the session
            hip_ops.obscalc(*[t.cuda() for t in pb["lame_true"]], stf, 1, ids, fn)
            hip_ops.forward(*m, stf, 0, ids, fn)
        syn_fn, syn_para = C.write_para(plain_of_w2(pb), "syn_store")      # no conditioning key, no W2 key: raw gathers, a directory of its own
        hip_ops.obscalc(*m, stf, 1, ids, syn_fn)
        syn = [np.ascontiguousarray(ft.read_shot_gather(syn_para["data_dir_name"], "ett", sid, pb["nSteps"])) for sid in G.shots_of(pb)]
        for p in (fn, tfn):
            for i, sid in enumerate(ids.tolist()):
                hip_ops.set_observed(p, sid, torch.from_numpy(np.ascontiguousarray(obs[i])))

        def twin_gradient():
            out = hip_ops.backward(*m, stf, 1, ids, tfn)
            return [t.cpu() for t in out[:4]], hip_ops.stats(tfn)["launches"]

        before = twin_gradient()
        whole = identical(syn, tag + " data_misfit")
        alone = identical(syn[one], tag + " data_misfit of shot %d alone" % k, obs=obs[one], ids=ids[one])
        f_lib, a_lib = H.call(hip_ops, pb, obs, syn)
        f_k = [H.call(hip_ops, pb, obs[i:i + 1], syn[i:i + 1], ids[i:i + 1]) for i in range(len(obs))]
        f0 = float(hip_ops.forward(*m, stf, 0, ids, fn)[0])
        bw = hip_ops.backward(*m, stf, 1, ids, fn)
        fb, g_ref = float(bw[0]), _np(bw[1:4])
        g_one = _np(hip_ops.backward(*m, stf, 1, ids[one], fn)[1:4]) if len(obs) > 1 else None
        ex = hip_ops.backward(*m, stf, 1, ids, fn, exact_adjoint=True)
        fe, g = float(ex[0]), _np(ex[1:4])
        again = _np(hip_ops.backward(*m, stf, 1, ids, fn, exact_adjoint=True)[1:4])
        wl = [{"ett": torch.from_numpy(np.ascontiguousarray(a)).cuda()} for a in a_lib]
        jta = _np(hip_ops.born_adjoint(*m, wl, stf, 1, ids, fn))
        born = [[x["ett"].cpu() for x in hip_ops.born(*m, *v, stf, 1, ids, p)] for p in (fn, tfn)]
        wd = [{"ett": torch.from_numpy(np.ascontiguousarray(x))} for x in ref["jd"]]
        jtw = [hip_ops.born_adjoint(*m, wd, stf, 1, ids, p) for p in (fn, tfn)]
        refused = []
        for name, run in (("gauss_newton exact", lambda: hip_ops.gauss_newton(*m, *v, stf, 1, ids, fn, exact=True)),
                          ("gauss_newton reference-style", lambda: hip_ops.gauss_newton(*m, *v, stf, 1, ids, fn, exact=False)),
                          ("data_gn", lambda: hip_ops.data_gn(flat(syn).cuda(), flat(syn).cuda(), ids, fn))):
            try:
                run()
                refused.append((name, None, "served"))
            except _native.SepFwiError as e:
                refused.append((name, e.code, str(e)))
        after = twin_gradient()
    fwi_ops.release()

    ka, kw = W.amplification(pb, obs, syn, O=oracle)
    print("%s: kappa_a %.1f kappa_W %.1f at the library's own gathers; the one shot %d of %d; peak |syn| %.1e; tie margin at the oracle's syn %.1e"
          % (tag, ka, kw, k, len(obs), max(float(np.abs(s).max()) for s in syn), o["margin"]))
    if not o["target"] or ka > W2_KAPPA_CAP:
        pytest.xfail("seed %d: no target -- the two oracle builds differ by %r, kappa_a %.1f (at the oracle's syn %.1f)" % (seed, o["yard"], ka, o["kappa_a"]))

    # 1. a_lib is right
    if whole is not None:
        check(whole[0] == f_lib and all(np.array_equal(x, y) for x, y in zip(whole[1], a_lib)), "a second data_misfit call differs")
        check(whole[2] > 0 and G.norm(whole[3]) > 0, "the reference's own adjoint source")
    if alone is not None:
        check(np.array_equal(alone[1][0], a_lib[k]), "the one-shot call has not the bits of the full call's rows of shot %d" % k)
        check(alone[0] == f_k[k][0] and (alone[0] > 0) == (alone[2] > 0), "the one-shot misfit")
    check(all(np.array_equal(fa[1][0], a_lib[i]) for i, fa in enumerate(f_k)), "a one-shot call's rows differ from the full call's")
    total = sum(float(fa[0]) for fa in f_k)
    print("%s: one-shot misfits %s sum to %.8e, the full call %.8e (gap %.2f EPS)" % (tag, " + ".join("%.8e" % fa[0] for fa in f_k), total, f_lib, abs(total - f_lib) / f_lib / EPS))
    check(f_lib > 0 and abs(total - f_lib) <= 4 * EPS * f_lib, "the one-shot misfits do not sum to the full one")
    if w["mode"] in ("window", "alone"):      # no filter: a dead trace is dead for every C, and its rows are 0, not small
        dead = [A == 0.0 for A in o["A"]]
        print("%s: dead traces per shot %r" % (tag, [int(x.sum()) for x in dead]))
        check(all(not np.any(x[z]) for x, z in zip(a_lib, dead)), "a dead trace's rows of the adjoint source are not 0")
    # 2. the passes use that misfit
    tol_f = (8.0 + 2.0 * kw) * EPS
    for name, f in (("forward", f0), ("backward", fb), ("exact backward", fe)):
        print("%s: misfit of %s %.8e, data_misfit of the library's own gathers %.8e (gap %.2f EPS, bound %.1f EPS)" % (tag, name, f, f_lib, abs(f - f_lib) / f_lib / EPS, tol_f / EPS))
        check(np.isfinite(f) and abs(f - f_lib) <= tol_f * f_lib, "misfit of %s" % name)
    # 3. the reference-style gradient against the oracle's backward pass with a_lib injected
    cases = [("", g_ref, w2_gradients(oracle, oracle_nvfma, o, a_lib))]
    if g_one is not None:
        cases.append((" of shot %d alone" % k, g_one, w2_gradients(oracle, oracle_nvfma, o, a_lib[one], one=True)))
    for what, arrs, sides in cases:
        for i, name in enumerate(GRADS):
            rg, ag = sides[0][name], sides[1][name]
            print("%s reference-style gradient%s %s: deviation from the oracle's pass with a_lib injected %.2e (the two oracle builds %.2e)"
                  % (tag, what, name, C.rel(C.d64(arrs[i], rg), rg), C.rel(C.d64(ag, rg), rg)))
            miss = C.gradient_miss(arrs[i], rg, ag, C.GRAD_TOL, 0.0, water)
            check(np.isfinite(arrs[i]).all() and C.l2(rg) > 0 and not miss, "reference-style gradient%s %s: %s" % (what, name, miss))
    # 4. the exact gradient
    omega = X.mask_omega(pb)
    check(all(np.isfinite(arr).all() and not np.any(arr[~omega]) for arr in g), "exact gradient outside Omega")
    check(all(np.array_equal(x, y) for x, y in zip(g, again)), "the second exact call of the session")
    tol_g = (16.0 + 2.0 * ka) * EPS
    for name, x, y in zip(GRADS, g, jta):
        gap = C.d64(x, -y) / max(C.l2(y), 1e-300)
        print("%s exact gradient %s against -J^T a_lib: rel-L2 %.2f EPS (bound %.1f EPS)" % (tag, name, gap / EPS, tol_g / EPS))
        check(C.l2(y) > 0 and gap <= tol_g, "exact gradient %s against -J^T a_lib" % name)
    na = G.norm(a_lib)
    for name, vec, key in (("v", o["v"], "jv"), ("d", o["dm"], "jd")):
        rr, aa = -G.dot(a_lib, ref[key]), -G.dot(a_lib, alt[key])
        cos = abs(rr) / max(na * G.norm(ref[key]), 1e-300)
        held(bad, X.model_dot(vec, g), rr, aa, tag + " <g, %s> against -<a_lib, J %s> (cosine %.3f)" % (name, name, cos), C.GRAD_TOL, 0.0,
             abs(rr) if cos >= COS else na * G.norm(ref[key]), name="cond")
    # 5. the rest of the interface
    check(born[0][k].abs().max() > 0 and all(torch.equal(x, y) for x, y in zip(*born)), "born under the keys")
    check(all(t.abs().max() > 0 for t in jtw[0]) and all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(*jtw)), "born_adjoint under the keys")
    for name, code, msg in refused:
        print("%s %s: code %r, %s" % (tag, name, code, msg[:160]))
        check(code == -1 and W.KEY in msg, "%s is not refused with the key's name" % name)
    print("%s: launches of a gradient call on the twin before %d and after %d" % (tag, before[1], after[1]))
    check(before[1] == after[1] and all(torch.equal(x, y) for x, y in zip(before[0], after[0])), "the twin file is touched")
    assert not bad, (tag, [what.replace(tag, "").strip() for what in bad])
