"""The reference for Gauss-Newton and the exact adjoint under windowed and band-passed data (include/sepfwi.h: sepfwi_condition, the
conditioned modes of sepfwi_born / sepfwi_adjoint_exact), outside the GPU.

Nothing adjoint is restated.  J is tests/born_ref.py (through tests/exact_adjoint_ref.py), and the data-space operators are the oracle's
own: C = cond_bandpass . cond_window as oracle.conditioned_residual composes them on a gather, Z the zeroing of time sample 0.  C^T is
only ever FORMED on the oracle side ("band-pass, then window") to show that it is the transpose (tests/test_conditioned_gn_reference.py);
the GPU identities need C alone:
    v^T H v = |Z C J v|^2        u^T H v = <Z C J u, Z C J v>        <g, v> = -<Z C J v, Z (C obs - C syn)>
Either oracle build serves (float64 transforms on the plain one, float32 on nvfma): their difference is the suite's yardstick.

The files (linear_problem): most of the signal's energy lies on a ramp of the filter (corners), the windows cut through the arrivals, and
the channel weights are 0.5 ... 2 with src_weight != 1 -- so that C C d, C d and d differ by far more than 10 % and a pass that applies C once
instead of twice, or not at all, cannot go unnoticed (inputs_discriminate asserts it for every J v a test uses)."""
import json
import os

import numpy as np

import exact_adjoint_ref as X
import problems as P
from born_ref import ROW

SMALL = dict(nz=40, nx=48, nPml=10, nSteps=120, nshots=2)      # the small problem of the Born and exact-adjoint tests
MODES = ("filter", "window", "both")                           # the three linear modes
ALL_MODES = MODES + ("narrow",)                                # ... and a narrow low band alone, the file on which Z shows (narrow)
NARROW = (0.0, 0.2, 0.2, 0.4)                                  # x f0
CORNERS = (0.3, 0.9, 1.1, 2.0)                                 # x f0 (corners)
COND_KEYS = ("if_win", "filter", "if_cross_misfit", "if_src_update")


def corners(f0):
    """[0.3, 0.9, 1.1, 2.0] f0.  On the small problem the record ends while the direct wave is still arriving at the fibre (120 steps, the
    source's delay alone is 48): the scattered gathers are a truncated onset whose spectrum falls monotonically from 0 Hz, so most of their
    energy lies on the filter's LOWER ramp and below it -- |B d| is 0.36 |d| and |B B d| 0.69 |B d| (inputs_discriminate prints them)."""
    return [c * f0 for c in CORNERS]


def narrow(f0):
    """[0, 0.2, 0.2, 0.4] f0, the kind of band a multi-scale inversion starts with.  Its impulse response is as long as the record, so
    that the band-passed arrival reaches back to time sample 0: 0.8 % of |C J v|^2 sits in that one sample, and a pass that forgets Z is
    off by that much (under the wider band of `corners` by 7e-6, which no tolerance sees)."""
    return [c * f0 for c in NARROW]


def windows(pb, sv, seed=5, error1=None):
    """Per-channel windows that cut through the arrival (the direct wave reaches the fibre in the record's last tenth): starts spread over
    the time before and into its onset, ends inside it, before the record's end; weights 0.5 ... 2; src_weight 3, 3.5, ... (large enough that the window's gain and the filter's loss do not cancel in |C C d| / |C d|)  error1 = (shot, channel): that channel's
    window is empty ("Window error 1": its trace stays untouched)."""
    rng = np.random.default_rng(seed)
    T = pb["nSteps"] * float(pb["para"]["dt"])
    sv = dict(sv)
    for k in [int(i) for i in pb["Shot_ids"].tolist()]:
        sh = dict(sv["shot%d" % k])
        n = int(sh["nrec"])
        sh["win_start"] = [float(v) for v in rng.uniform(0.60 * T, 0.93 * T, n)]
        sh["win_end"] = [float(v) for v in rng.uniform(0.95 * T, 0.995 * T, n)]
        sh["weights"] = [float(v) for v in rng.uniform(0.5, 2.0, n)]
        sh["src_weight"] = 3.0 + 0.5 * k
        if error1 is not None and error1[0] == k:
            sh["win_end"][error1[1]] = sh["win_start"][error1[1]]
        sv["shot%d" % k] = sh
    return sv


def write_files(pb, name, para, survey):
    """A parameter / survey file pair next to pb's own (a session of its own).  -> the parameter file's name"""
    here = os.path.dirname(pb["para_fname"])
    para = dict(para, survey_fname=os.path.join(here, name + "_survey.json"), data_dir_name=os.path.join(here, name + "_Data"))
    os.makedirs(para["data_dir_name"], exist_ok=True)
    with open(para["survey_fname"], "w") as fp:
        json.dump(survey, fp)
    fn = os.path.join(here, name + ".json")
    with open(fn, "w") as fp:
        json.dump(para, fp)
    return fn, para


def set_mode(pb, mode, name=None, error1=None, **keys):
    """pb with the conditioning keys of `mode` ("filter", "window", "both", "narrow", "none") in pb["para"] / pb["survey"], written as a file pair
    of their own: pb["para_fname"] names it.  The windows are in the survey in every mode (without if_win nobody reads them).
    -> a shallow copy of pb"""
    pb = dict(pb)
    para = {k: v for k, v in pb["para"].items() if k not in COND_KEYS}
    if mode in ("filter", "both"):
        para["filter"] = corners(float(para["f0"]))
    if mode == "narrow":
        para["filter"] = narrow(float(para["f0"]))
    if mode in ("window", "both"):
        para["if_win"] = True
    para.update(keys)
    sv = windows(pb, pb["survey"], error1=error1)
    pb["para_fname"], pb["para"] = write_files(pb, name or mode, para, sv)
    pb["survey"], pb["survey_fname"] = sv, pb["para"]["survey_fname"]
    pb["data_dir"] = pb["para"]["data_dir_name"]
    return pb


def linear_problem(tmp, mode, **kw):
    return set_mode(P.make_problem(str(tmp), **dict(SMALL, **kw)), mode)


def C_of(O, pb, d, sid):
    """C on one shot's (nrec, nSteps) gather, as oracle.conditioned_residual applies it to a synthetic gather"""
    cond = O.conditioning_of(pb["para"], pb["survey"], int(sid))
    d = np.asarray(d, np.float32)
    if cond is None:
        return d.copy()
    out = O.cond_window(d, float(pb["para"]["dt"]), cond["win"])
    if cond.get("filter") is not None:
        out = O.cond_bandpass(out, float(pb["para"]["dt"]), cond["filter"])
    return out


def Ct_of(O, pb, d, sid):
    """band-pass, then window: what the chain applies to the residual"""
    cond = O.conditioning_of(pb["para"], pb["survey"], int(sid))
    out = np.asarray(d, np.float32)
    if cond is None:
        return out.copy()
    if cond.get("filter") is not None:
        out = O.cond_bandpass(out, float(pb["para"]["dt"]), cond["filter"])
    return O.cond_window(out, float(pb["para"]["dt"]), cond["win"])


def Z(d):
    out = np.array(d, copy=True)
    out[..., 0] = 0.0
    return out


def shots_of(pb):
    return [int(i) for i in pb["Shot_ids"].tolist()]


def C_all(O, pb, gathers, op=C_of):
    """per shot: a list (or stacked array) of (nrec, nSteps) -> list"""
    return [op(O, pb, g, sid) for g, sid in zip(gathers, shots_of(pb))]


def dot(a, b):
    return sum(float((np.asarray(x, np.float64) * np.asarray(y, np.float64)).sum()) for x, y in zip(a, b))


def norm(a):
    return float(np.sqrt(dot(a, a)))


def jv_ett(lib, pb, v, dStf=None):
    """born_ref's scattered axial strain, per shot a (nrec, nSteps) float32 array (the shots may differ in their channel counts);
    dStf: + J_s ds, the oracle's gathers for the source ds (the wavefield is linear in the source: tests/stf_ref.py)"""
    import born_ref as B
    m = [t.numpy() for t in pb["lame_init"]]
    plain = {k: val for k, val in pb["para"].items() if k not in COND_KEYS}
    out = [np.zeros((int(pb["survey"]["shot%d" % s]["nrec"]), pb["nSteps"]), np.float32) for s in shots_of(pb)]
    if v is not None:
        r = B.born(lib, *m, *v, pb["Stf"].numpy(), pb["Shot_ids"].numpy(), plain, pb["survey"], stack=False)["dsyn"]
        out = [a[ROW["ett"]] for a in r]
    if dStf is not None:
        import stf_ref as S
        js = S.js_ref(lib, m, dStf, pb["Shot_ids"].numpy(), plain, pb["survey"])
        out = [(a.astype(np.float64) + b["ett"]).astype(np.float32) for a, b in zip(out, js)]
    return out


def inputs_discriminate(O, pb, jv, what):
    """The conditions on a test's own inputs: |C C Jv| differs from |C Jv| and |C Jv| from |Jv| by more than 10 %."""
    c1 = C_all(O, pb, jv)
    c2 = C_all(O, pb, c1)
    n0, n1, n2 = norm(jv), norm(c1), norm(c2)
    print("conditioned GN inputs %s: |Jv| %.4e, |C Jv| %.4e (%.3f of it), |C C Jv| %.4e (%.3f of |C Jv|)" % (what, n0, n1, n1 / n0, n2, n2 / n1))
    assert n0 > 0 and abs(n1 / n0 - 1.0) > 0.10 and abs(n2 / n1 - 1.0) > 0.10, (what, n0, n1, n2)
    return c1


def discrimination(O, pb, gathers):
    """inputs_discriminate for several gathers at once, without the assertion: gathers {name: per-shot list}
    -> ({name: (|C d| / |d|, |C C d| / |C d|)}, whether every ratio differs from 1 by more than 10 %)"""
    out = {}
    for name, d in gathers.items():
        c1 = C_all(O, pb, d)
        c2 = C_all(O, pb, c1)
        n0, n1, n2 = norm(d), norm(c1), norm(c2)
        out[name] = (n1 / n0, n2 / n1) if n0 > 0 and n1 > 0 else (1.0, 1.0)
    return out, all(abs(r - 1.0) > 0.10 for pair in out.values() for r in pair)


def oracle_gathers(lib, pb, model):
    """the oracle's raw axial-strain gathers of a model, per shot (nrec, nSteps) float32, and all four components for cufd's obs"""
    plain = {k: val for k, val in pb["para"].items() if k not in COND_KEYS}
    m = [t.numpy() for t in pb[model]]
    full = [lib.cufd(*m, pb["Stf"].numpy(), 2, np.asarray([s], np.int32), plain, pb["survey"])["syn"][0] for s in shots_of(pb)]
    return [a[ROW["ett"]] for a in full], full


def conditioned_residual(lib, pb, obs, syn):
    """Z (C obs - C syn) per shot in float64, and the conditioned misfit 1/2 |.|^2"""
    r = [Z(C_of(lib, pb, o, s).astype(np.float64) - C_of(lib, pb, y, s).astype(np.float64)) for o, y, s in zip(obs, syn, shots_of(pb))]
    return r, 0.5 * dot(r, r)


held = X.held
