"""The robust misfits through the passes, on the GPU (-m gpu): parameter keys robust_misfit / robust_delta under sepfwi_cufd (calc_id 0 and
1, the persistent loop and the two-launch step), sepfwi_adjoint_exact (gradient mode and the product), sepfwi_born's product, the refusals,
and what a file without the key keeps.

Problem: problems.cond_problem's sizes (44 x 60, 300 steps, two shots, its windows and weights) under the key alone and with filter and
if_win (envelope_ref.gpu_problem with these keys), and the same survey with GENERAL receivers (tests/test_gpu_w2_misfit.py's), so that the
adjoint source goes through the injection plans.  The observed gathers are the oracle's of the true model with TEN SPIKES of 100 x the
trace's peak written into every trace; robust_delta = 0.1, so that the spikes and a part of the clean residual lie outside.

By chain of custody, as tests/test_gpu_w2_misfit.py:
  1  the misfit of calc_id 0 and 1 equals data_misfit(obs, syn) on the library's OWN synthetic gathers (obscalc of the same model into a
     second directory) bit for bit: the same kernels on the same gathers, the shots summed in the same order
  2  the reference-style gradient equals the oracle's backward pass with adj_src = the reference's a at those gathers (tests/robust_ref.py,
     C and C^T the oracle's), to the suite's 1e-3 |g| + 3 x the two oracle builds' difference
  3  the exact gradient equals -J^T a, J^T the w mode of sepfwi_adjoint_exact and a data_misfit's at those gathers: the same kernels on the
     same residual buffer when the gathers agree bit for bit; a gather off by one float32 rounding moves a by as much (psi is
     1-Lipschitz in r: nothing amplifies), well inside the 1e-5 |g| that tests/test_gpu_w2_misfit.py allows its amplifying map
  4  <g_exact, v> = -<a, J v>, J from tests/born_ref.py on both oracle builds, to the exact adjoint's tolerances (exact_adjoint_ref.held)
  5  the product with exact=True: v^T H v = |W^1/2 Z C J v|^2 and u^T H v = v^T H u, W the reference's IRLS weight at (C obs, C syn)
Every comparison prints its deviation before it asserts; profiles/r29_robust_misfit.txt holds the figures measured on the MI355X.

On the parent commit the keys are unknown: every call under them fails."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import cond_gn_ref as G
import envelope_ref as E
import exact_adjoint_ref as X
import problems as P
import robust_ref as R
from exact_adjoint_ref import cuda, held
from fuzz_common import GRAD_TOL, array_held, d64, l2, write_para
from sepfwi import utils as ft

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
GRADS = ("gLambda", "gMu", "gDen")
OPTIONS = {"default": dict(), "two_launch": dict(bwd_fuse=2)}
DELTA, SPIKES = 0.1, 10
SIDES = {"huber_alone": ("huber", "alone", False), "cauchy_both": ("cauchy", "both", False), "huber_general": ("huber", "both", True)}


def model(pb, which="lame_init"):
    return [t.cuda() for t in pb[which]]


def flat(gathers):
    return torch.from_numpy(np.concatenate([np.asarray(g, np.float32).reshape(-1) for g in gathers]))


def robust_problem(tmp, keys, kind="huber", name=None, key=True, **more):
    """envelope_ref.gpu_problem under this misfit's keys"""
    extra = {R.KEY: kind, R.DELTA_KEY: DELTA} if key else {}
    extra.update(more)
    return E.gpu_problem(tmp, keys, name=name or ("robust_" + keys), key=False, **extra)


def plain(pb):
    """pb with the conditioning keys and this misfit's keys out of its parameter dict"""
    return dict(pb, para={k: v for k, v in pb["para"].items() if k not in R.STRIP})


def generalise(pb):
    """the survey of pb with general receivers, written over pb's survey file (tests/test_gpu_w2_misfit.py's)"""
    sv = json.loads(json.dumps(pb["survey"]))
    s0, s1 = sv["shot0"], sv["shot1"]
    s0["z_rec"] = [z - (i % 2) for i, z in enumerate(s0["z_rec"])]
    idx = list(range(3, int(s1["nrec"]), 3))
    for k in ("z_rec", "x_rec", "win_start", "win_end", "weights"):
        s1[k] = [s1[k][i] for i in idx]
    s1["z_rec"] = [z - 2 * (i % 3) for i, z in enumerate(s1["z_rec"])]
    s1["nrec"] = len(idx)
    with open(pb["para"]["survey_fname"], "w") as fp:
        json.dump(sv, fp)
    return dict(pb, survey=sv)


def spiked(gathers, rng):
    out = []
    for g in gathers:
        g = np.array(g, np.float32)
        for r in range(g.shape[0]):
            idx = 1 + rng.choice(g.shape[1] - 1, size=SPIKES, replace=False)
            g[r, idx] = (np.float32(100.0) * np.abs(g[r]).max() * rng.choice([-1.0, 1.0], size=SPIKES)).astype(np.float32)
        out.append(g)
    return out


class Side:
    """one file: the problem, the oracle's raw gathers of lame_true with spikes (obs), the library's own raw gathers of lame_init (syn), and
    data_misfit of the two"""

    def __init__(self, hip_ops, lib, tmp, kind, keys, general):
        self.kind, self.keys = kind, keys
        self.pb = pb = robust_problem(tmp, keys, kind)
        if general:
            self.pb = pb = generalise(pb)
        clean, _ = G.oracle_gathers(lib, pb, "lame_true")
        self.obs = spiked(clean, np.random.default_rng(41))
        hip_ops.release()
        fn, para = write_para(plain(pb), "syn_store")      # no conditioning key: raw gathers, a directory of its own
        hip_ops.obscalc(*model(pb), pb["Stf"], 1, pb["Shot_ids"], fn)
        self.syn = [np.ascontiguousarray(ft.read_shot_gather(para["data_dir_name"], "ett", sid, pb["nSteps"])) for sid in G.shots_of(pb)]
        f, a = hip_ops.data_misfit(flat(self.obs).cuda(), flat(self.syn).cuda(), pb["Shot_ids"], pb["para_fname"])
        self.f, off, self.a = f, 0, []
        for g in self.obs:
            self.a.append(a[off:off + g.size].view(*g.shape).cpu().numpy())
            off += g.size
        hip_ops.release()

    def install(self, hip_ops, pb=None):
        pb = pb or self.pb
        for i, sid in enumerate(G.shots_of(pb)):
            hip_ops.set_observed(pb["para_fname"], sid, torch.from_numpy(np.ascontiguousarray(self.obs[i])))


@pytest.fixture(scope="module")
def sides(oracle, hip_ops, tmp_path_factory):
    """computed once, left unchanged"""
    return {k: Side(hip_ops, oracle, tmp_path_factory.mktemp("robust_" + k), *v) for k, v in SIDES.items()}


# ---- 1: the misfit of a misfit call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", list(SIDES))
def test_misfit_call_equals_data_misfit_of_its_own_gathers(hip_ops, sides, side):
    s = sides[side]
    pb = s.pb
    hip_ops.release()
    s.install(hip_ops)
    f0 = float(hip_ops.forward(*model(pb), pb["Stf"], 0, pb["Shot_ids"], pb["para_fname"])[0])
    f1 = float(hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])[0])
    l2_f, _ = hip_ops.data_misfit(flat(s.obs).cuda(), flat(s.syn).cuda(), pb["Shot_ids"], robust_problem(pb["para_fname"].rsplit("/", 1)[0] + "/l2", s.keys, key=False)["para_fname"]) \
        if side != "huber_general" else (float("nan"), None)
    print("robust 1 %s: calc_id 0 %.8e, calc_id 1 %.8e, data_misfit of the library's own gathers %.8e (gaps %.2f and %.2f EPS); the L2 misfit of the same gathers %.4e"
          % (side, f0, f1, s.f, abs(f0 - s.f) / s.f / EPS, abs(f1 - s.f) / s.f / EPS, l2_f))
    assert s.f > 0 and f0 == s.f and f1 == s.f
    hip_ops.release()


# ---- 2: the reference-style gradient, line and general receivers, the loop and the two-launch step -------------------------------------------
@pytest.mark.parametrize("opts", list(OPTIONS))
@pytest.mark.parametrize("side", list(SIDES))
def test_reference_style_gradient(oracle, oracle_nvfma, hip_ops, sides, side, opts):
    s = sides[side]
    pb = s.pb
    if not hasattr(s, "grad"):      # once per side: the reference's a at the library's gathers, through the oracle's backward pass, both builds
        s.ref = [R.data_misfit(lib, pb, s.obs, s.syn) for lib in (oracle, oracle_nvfma)]
        s.grad = [E.gradient(lib, plain(pb), r[1]) for lib, r in zip((oracle, oracle_nvfma), s.ref)]
    print("robust 2 %s: the reference's a against data_misfit's: rel-L2 %.2e (the two oracle builds %.2e); misfit gap %.2e"
          % (side, G.norm([x.astype(np.float64) - y for x, y in zip(s.a, s.ref[0][1])]) / G.norm(s.ref[0][1]),
             G.norm([x.astype(np.float64) - y for x, y in zip(s.ref[1][1], s.ref[0][1])]) / G.norm(s.ref[0][1]), abs(s.f - s.ref[0][0]) / s.ref[0][0]))
    hip_ops.release()
    with P.kernel_options(**OPTIONS[opts]):
        s.install(hip_ops)
        out = hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    got = dict(zip(GRADS + ("gStf",), [t.cpu().numpy() for t in out[1:5]]))
    for name in GRADS + ("gStf",):
        ref, alt = s.grad[0][name], s.grad[1][name]
        g = got[name][:ref.shape[0]] if name == "gStf" else got[name]
        print("robust 2 %s %s %s: rel-L2 %.2e (the two oracle builds %.2e)" % (side, opts, name, d64(g, ref) / l2(ref), d64(alt, ref) / l2(ref)))
        assert l2(ref) > 0 and array_held(g, ref, alt, GRAD_TOL), (side, opts, name)
    hip_ops.release()


# ---- 3, 4: the exact gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["huber_alone", "cauchy_both"])
def test_exact_gradient(oracle, oracle_nvfma, hip_ops, sides, side):
    s = sides[side]
    pb = s.pb
    hip_ops.release()
    s.install(hip_ops)
    m = model(pb)
    out = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact_adjoint=True)
    f, g = float(out[0]), [t.cpu().numpy() for t in out[1:4]]
    print("robust 3 %s: misfit of the exact pass %.8e, data_misfit %.8e" % (side, f, s.f))
    assert abs(f - s.f) <= 8 * EPS * s.f
    X.outside_is_zero(pb, g, "exact robust gradient " + side)
    w = [{"ett": torch.from_numpy(a).cuda()} for a in s.a]
    jt = [t.cpu().numpy() for t in hip_ops.born_adjoint(*m, w, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])]
    for name, x, y in zip(GRADS, g, jt):
        gap = d64(x, -y) / l2(y)
        print("robust 3 %s %s: exact gradient against -J^T a: rel-L2 %.2e" % (side, name, gap))
        assert l2(y) > 0 and gap <= 1e-5, (side, name)
    v = X.smooth_v(pb, 3)
    jv = [G.jv_ett(lib, plain(pb), v) for lib in (oracle, oracle_nvfma)]
    rr, aa = -G.dot(s.a, jv[0]), -G.dot(s.a, jv[1])
    held(X.model_dot(v, g), rr, aa, "robust 4 %s <g, v> = -<a, J v>" % side, scale=abs(rr))
    hip_ops.release()


# ---- 5: the products ----------------------------------------------------------------------------------------------------------------------------
def gn(hip_ops, pb, v, exact=True):
    return [h.cpu().numpy() for h in hip_ops.gauss_newton(*model(pb), *cuda(v), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact=exact)]


@pytest.mark.parametrize("side", ["huber_alone", "cauchy_both"])
def test_exact_product(oracle, oracle_nvfma, hip_ops, sides, side):
    """gauss_newton(exact=True): v^T H v = |W^1/2 Z C J P v|^2 and u^T H v = v^T H u = <W^1/2 Z C J u, W^1/2 Z C J v>, W the reference's
    IRLS weight at (C obs, C of the background gather); the call reads the observed gathers from the session's store"""
    s = sides[side]
    pb = s.pb
    hip_ops.release()
    s.install(hip_ops)
    vs = [X.smooth_v(pb, 3), X.smooth_v(pb, 4)]
    ids = G.shots_of(pb)
    z = []
    for lib in (oracle, oracle_nvfma):
        c = lambda gs: [R.C_of(lib, pb, g, sid) for g, sid in zip(gs, ids)]
        _, _, ws, _ = R.conditioned_misfit(pb, c(s.obs), c(s.syn))
        z.append([[np.sqrt(w) * x.astype(np.float64) for w, x in zip(ws, c(G.jv_ett(lib, plain(pb), v)))] for v in vs])
    hv = [gn(hip_ops, pb, v) for v in vs]
    uhu = [X.model_dot(vs[k], hv[k]) for k in range(2)]
    for k in range(2):
        X.outside_is_zero(pb, hv[k], side)
        held(uhu[k], G.dot(z[0][k], z[0][k]), G.dot(z[1][k], z[1][k]), "robust 5 %s v^T H v, %d" % (side, k))
    scale = float(np.sqrt(uhu[0] * uhu[1]))
    c21, c12 = X.model_dot(vs[1], hv[0]), X.model_dot(vs[0], hv[1])
    cr, ca = G.dot(z[0][0], z[0][1]), G.dot(z[1][0], z[1][1])
    held(c21, c12, c12 + (ca - cr), "robust 5 %s symmetry" % side, scale=scale)
    held(c21, cr, ca, "robust 5 %s cross term against the reference" % side, scale=scale)
    l2file = robust_problem(pb["para_fname"].rsplit("/", 1)[0] + "/l2prod", s.keys, key=False)
    h2 = gn(hip_ops, l2file, vs[0])
    print("robust 5 %s: v^T H v under the key %.6e, under the L2 file %.6e (the weight is in (0, 1])" % (side, uhu[0], X.model_dot(vs[0], h2)))
    assert 0 < uhu[0] < X.model_dot(vs[0], h2)
    hip_ops.release()


def test_reference_style_product_runs_and_is_weighted(hip_ops, sides):
    """gauss_newton(exact=False) under the key: finite, non-zero, and not the L2 file's product"""
    s = sides["huber_alone"]
    pb = s.pb
    hip_ops.release()
    s.install(hip_ops)
    v = X.smooth_v(pb, 3)
    hv = gn(hip_ops, pb, v, exact=False)
    h2 = gn(hip_ops, robust_problem(pb["para_fname"].rsplit("/", 1)[0] + "/l2ref", s.keys, key=False), v, exact=False)
    gaps = [d64(a, b) / l2(b) for a, b in zip(hv, h2)]
    print("robust 5 reference-style product against the L2 file's: rel-L2 %s" % " ".join("%.3f" % x for x in gaps))
    assert all(np.isfinite(a).all() and l2(a) > 0 for a in hv) and all(x > 1e-2 for x in gaps)
    hip_ops.release()


def test_gauss_newton_cg_under_the_key(hip_ops, sides):
    """three inner iterations of obj_wrapper.gauss_newton_cg on the exact IRLS product, unchanged: it completes, and the quadratic model
    q(p) = <g, p> + 1/2 <p, H p> decreases monotonically over the iterates (H is symmetric and non-negative)."""
    from sepfwi.obj_wrapper import gauss_newton_cg
    s = sides["cauchy_both"]
    pb = s.pb
    hip_ops.release()
    s.install(hip_ops)
    m = model(pb)
    g = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact_adjoint=True)[1:4]
    hessvec = lambda v: hip_ops.gauss_newton(*m, *v, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact=True)
    dot = lambda a, b: float(sum((x.double() * y.double()).sum() for x, y in zip(a, b)))
    q = [0.0]
    for n in (1, 2, 3):
        p, hist = gauss_newton_cg(hessvec, g, maxiter=n, rtol=0.0)
        assert len(hist) == n + 1 and all(np.isfinite(h) for h in hist)
        q.append(dot(g, p) + 0.5 * dot(p, hessvec(tuple(p))))
    print("robust 5: quadratic model over three conjugate-gradient iterations %s, residual history %s" % (["%.6e" % x for x in q], ["%.3e" % h for h in hist]))
    assert all(b < a for a, b in zip(q[:-1], q[1:])), q
    hip_ops.release()


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------------------
BAD = {"if_cross_misfit": {"if_cross_misfit": True}, "if_envelope_misfit": {"if_envelope_misfit": True}, "if_w2_misfit": {"if_w2_misfit": True},
       "if_src_update": {"if_src_update": True}, "misfit_w_vx": {"misfit_w_vx": 0.5},
       "kind": {R.KEY: "l1"}, "delta_zero": {R.DELTA_KEY: 0.0}, "delta_negative": {R.DELTA_KEY: -1.0}, "quantile_zero": {R.Q_KEY: 0.0}, "quantile_two": {R.Q_KEY: 2.0}}
NAMES = {"kind": R.KEY, "delta_zero": R.DELTA_KEY, "delta_negative": R.DELTA_KEY, "quantile_zero": R.Q_KEY, "quantile_two": R.Q_KEY, "no_delta": R.DELTA_KEY,
         "stray_delta": R.DELTA_KEY, "stray_quantile": R.Q_KEY}


@pytest.mark.parametrize("other", list(BAD) + ["no_delta", "stray_delta", "stray_quantile"])
def test_refusals_reach_the_c_abi(hip_ops, sides, other):
    """the key with each incompatible key, another kind, a bad or missing robust_delta, a bad robust_quantile, a stray robust_delta /
    robust_quantile: -1 (SEPFWI_EINVAL) and the key names, from a misfit call and from the data-space entry; the outputs keep their
    bits.  Before a session exists; a session of a good file works afterwards."""
    from sepfwi import _native
    L = _native.lib()
    s = sides["huber_alone"]
    hip_ops.release()
    here = s.pb["para_fname"].rsplit("/", 1)[0] + "/bad_" + other
    if other == "no_delta":
        bad = robust_problem(here, "alone", key=False, **{R.KEY: "huber"})
    elif other.startswith("stray"):
        bad = robust_problem(here, "alone", key=False, **{NAMES[other]: 0.5})
    else:
        bad = robust_problem(here, "alone", **BAD[other])
    m = model(bad)
    stf, ids = bad["Stf"].contiguous(), np.ascontiguousarray(bad["Shot_ids"].numpy(), dtype=np.int32)
    mis, adj = torch.full((1,), 7.0), torch.full((sum(g.size for g in s.obs),), 7.0)
    p = lambda t: C.c_void_p(t.data_ptr())
    x = torch.zeros(adj.numel())
    rcs = [L.sepfwi_cufd(p(mis), None, None, None, None, *[p(t) for t in m], p(stf), 0, 0, int(ids.size), C.c_void_p(ids.ctypes.data), bad["para_fname"].encode())]
    msgs = [L.sepfwi_last_error()]
    rcs.append(L.sepfwi_data_misfit(p(mis), p(adj), p(x), p(x), 0, int(ids.size), C.c_void_p(ids.ctypes.data), bad["para_fname"].encode(), None))
    msgs.append(L.sepfwi_last_error())
    rcs.append(L.sepfwi_data_gn_obs(p(adj), p(x), p(x), p(x), 0, int(ids.size), C.c_void_p(ids.ctypes.data), bad["para_fname"].encode(), None))
    msgs.append(L.sepfwi_last_error())
    print("robust 6 %s: %s %s" % (other, rcs, msgs[0]))
    for rc, msg in zip(rcs, msgs):
        if other in NAMES:
            assert rc == -1 and NAMES[other].encode() in msg, (rc, msg)
        else:
            assert rc == -1 and R.KEY.encode() in msg and other.encode() in msg, (rc, msg)
    assert float(mis[0]) == 7.0 and bool((adj == 7.0).all())      # nothing was touched
    s.install(hip_ops)
    f = float(hip_ops.forward(*model(s.pb), s.pb["Stf"], 0, s.pb["Shot_ids"], s.pb["para_fname"])[0])
    assert f == s.f
    hip_ops.release()


# ---- 7: untouched -----------------------------------------------------------------------------------------------------------------------------------
def live_bytes():
    from sepfwi import _native
    d, h = C.c_longlong(0), C.c_longlong(0)
    _native.check(_native.lib().sepfwi_debug_live_bytes(C.byref(d), C.byref(h)))
    return d.value, h.value


@pytest.mark.parametrize("side", ["huber_alone", "cauchy_both"])
def test_a_file_without_the_key_is_untouched(hip_ops, sides, side):
    """the same file without the key: launches, device_bytes and output bits of a gradient call and of an exact Born product before and
    after a session under the key ran a gradient call, a product and the data-space entries in the same process; under the key a gradient
    call costs one launch per shot more where the file had its conditioner (the residual kernel's one becomes select-and-residual plus the
    sum); live device bytes return to their start after release."""
    s = sides[side]
    keyed = s.pb
    unkeyed = robust_problem(keyed["para_fname"].rsplit("/", 1)[0] + "/untouched", s.keys, key=False)
    v = X.smooth_v(keyed, 3)
    hip_ops.release()
    start = live_bytes()

    def run(pb):
        s.install(hip_ops, pb)
        out = hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
        st = hip_ops.stats(pb["para_fname"])
        hv = hip_ops.gauss_newton(*model(pb), *cuda(v), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact=True)
        sp = hip_ops.stats(pb["para_fname"])
        return list(out) + list(hv), st["launches"], sp["device_bytes"], sp["launches"]      # (the bytes once the product's buffers exist)

    before = run(unkeyed)
    with_key = run(keyed)
    hip_ops.data_misfit(flat(s.obs).cuda(), flat(s.syn).cuda(), keyed["Shot_ids"], keyed["para_fname"])
    hip_ops.data_gn(flat(s.syn).cuda(), flat(s.syn).cuda(), keyed["Shot_ids"], keyed["para_fname"], obs=flat(s.obs).cuda())
    after = run(unkeyed)
    print("robust 7 %s: launches of a gradient call without the key %d and %d, under the key %d; of a product %d and %d, under the key %d; device bytes %d, %d, %d"
          % (side, before[1], after[1], with_key[1], before[3], after[3], with_key[3], before[2], after[2], with_key[2]))
    assert before[1:] == after[1:], (before[1:], after[1:])
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(before[0], after[0]))
    if s.keys == "both":
        assert with_key[1] == before[1] + len(G.shots_of(keyed))
    hip_ops.release()
    assert live_bytes() == start
