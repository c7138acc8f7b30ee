"""The W2 misfit through the passes, on the GPU (-m gpu): parameter key if_w2_misfit under sepfwi_cufd (calc_id 0 and 1, the persistent loop
and the two-launch step), sepfwi_adjoint_exact (gradient mode), the refusals, and what a file without the key keeps.

Problem: problems.cond_problem's sizes (44 x 60, 300 steps, two shots, its windows and weights) under the key alone, with filter, with
if_win, with both (envelope_ref.gpu_problem with this key), and the same survey with GENERAL receivers: shot 0's channels on alternating
rows, shot 1 every third channel on three rows, so that the adjoint source goes through the injection plans.

The map from the gathers to the adjoint source amplifies a relative input error by up to 1e2 (tests/test_w2_reference.py), so the passes
are held by chain of custody, not by re-deriving the adjoint source from the oracle's gathers:
  1  the misfit of calc_id 0 equals data_misfit(obs, syn) on the library's OWN synthetic gathers (obscalc of the same model into a second
     directory) to 8 x 2^-24, the bound tests/test_gpu_w2_data.py holds data_misfit to
  2  the reference-style gradient equals the oracle's backward pass with adj_src = the reference's a at those gathers (tests/w2_ref.py,
     C and C^T the oracle's; envelope_ref.gradient's hook), to the suite's 1e-3 |g| + 3 x the two oracle builds' difference
  3  the exact gradient under the key equals -J^T a, J^T the w mode of sepfwi_adjoint_exact and a data_misfit's at those gathers.  Both
     passes run the same kernels on the same residual buffer when their gathers agree bit for bit, and then agree bit for bit; gathers that
     differ by one float32 rounding (2^-24) would move a, and with it g, by 1e2 x 2^-24 = 6e-6: the bound is 1e-5 |g|
  4  <g_exact, v> = -<a, J v>, J from tests/born_ref.py on both oracle builds, to the exact adjoint's tolerances (exact_adjoint_ref.held)
Every comparison prints its deviation before it asserts; profiles/r28_w2_misfit.txt holds the figures measured on the MI355X.

On the parent commit the key is ignored and the L2 misfit comes back: every comparison fails there."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import cond_gn_ref as G
import envelope_ref as E
import exact_adjoint_ref as X
import problems as P
import w2_ref as W
from exact_adjoint_ref import cuda, held
from fuzz_common import GRAD_TOL, array_held, d64, l2, write_para
from sepfwi import utils as ft

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
GRADS = ("gLambda", "gMu", "gDen")
OPTIONS = {"default": dict(), "two_launch": dict(bwd_fuse=2)}


def model(pb, which="lame_init"):
    return [t.cuda() for t in pb[which]]


def flat(gathers):
    return torch.from_numpy(np.concatenate([np.asarray(g, np.float32).reshape(-1) for g in gathers]))


def w2_problem(tmp, keys, name=None, key=True, **more):
    """envelope_ref.gpu_problem under this misfit's key"""
    extra = dict(more)
    if key:
        extra[W.KEY] = True
    return E.gpu_problem(tmp, keys, name=name or ("w2_" + keys), key=False, **extra)


def plain(pb):
    """pb with the conditioning keys and this misfit's keys out of its parameter dict"""
    return dict(pb, para={k: v for k, v in pb["para"].items() if k not in W.STRIP})


def generalise(pb):
    """the survey of pb with general receivers, written over pb's survey file (a directory of its own)"""
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


class Side:
    """one key set: the problem, the oracle's raw gathers of lame_true (obs), the library's own raw gathers of lame_init (syn), and
    data_misfit of the two"""

    def __init__(self, hip_ops, lib, tmp, keys, general=False):
        self.keys = keys
        self.pb = pb = w2_problem(tmp, keys)
        if general:
            self.pb = pb = generalise(pb)
        self.obs, _ = G.oracle_gathers(lib, pb, "lame_true")
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
    out = {k: Side(hip_ops, oracle, tmp_path_factory.mktemp("w2_" + k), k) for k in E.KEYSETS}
    out["general"] = Side(hip_ops, oracle, tmp_path_factory.mktemp("w2_general"), "both", general=True)
    return out


# ---- 1: the misfit of a misfit call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", list(E.KEYSETS) + ["general"])
def test_misfit_call_equals_data_misfit_of_its_own_gathers(hip_ops, sides, keys):
    s = sides[keys]
    pb = s.pb
    hip_ops.release()
    s.install(hip_ops)
    f0 = float(hip_ops.forward(*model(pb), pb["Stf"], 0, pb["Shot_ids"], pb["para_fname"])[0])
    f1 = float(hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])[0])
    print("w2 1 %s: calc_id 0 %.8e, calc_id 1 %.8e, data_misfit of the library's own gathers %.8e (gaps %.2f and %.2f EPS)"
          % (keys, f0, f1, s.f, abs(f0 - s.f) / s.f / EPS, abs(f1 - s.f) / s.f / EPS))
    assert s.f > 0 and abs(f0 - s.f) <= 8 * EPS * s.f and abs(f1 - s.f) <= 8 * EPS * s.f
    hip_ops.release()


# ---- 2, 8: the reference-style gradient, line and general receivers, the loop and the two-launch step ----------------------------------------
@pytest.mark.parametrize("opts", list(OPTIONS))
@pytest.mark.parametrize("keys", ["alone", "both", "general"])
def test_reference_style_gradient(oracle, oracle_nvfma, hip_ops, sides, keys, opts):
    s = sides[keys]
    pb = s.pb
    if not hasattr(s, "grad"):      # once per side: the reference's a at the library's gathers, through the oracle's backward pass, both builds
        s.ref = [W.data_misfit(lib, pb, s.obs, s.syn) for lib in (oracle, oracle_nvfma)]
        s.grad = [E.gradient(lib, plain(pb), r[1]) for lib, r in zip((oracle, oracle_nvfma), s.ref)]
    print("w2 2 %s: the reference's a against data_misfit's: rel-L2 %.2e (the two oracle builds %.2e); misfit gap %.2e"
          % (keys, G.norm([x.astype(np.float64) - y for x, y in zip(s.a, s.ref[0][1])]) / G.norm(s.ref[0][1]),
             G.norm([x.astype(np.float64) - y for x, y in zip(s.ref[1][1], s.ref[0][1])]) / G.norm(s.ref[0][1]), abs(s.f - s.ref[0][0]) / s.ref[0][0]))
    hip_ops.release()
    with P.kernel_options(**OPTIONS[opts]):
        s.install(hip_ops)
        out = hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    got = dict(zip(GRADS + ("gStf",), [t.cpu().numpy() for t in out[1:5]]))
    for name in GRADS + ("gStf",):
        ref, alt = s.grad[0][name], s.grad[1][name]
        g = got[name][:ref.shape[0]] if name == "gStf" else got[name]
        print("w2 2 %s %s %s: rel-L2 %.2e (the two oracle builds %.2e)" % (keys, opts, name, d64(g, ref) / l2(ref), d64(alt, ref) / l2(ref)))
        assert l2(ref) > 0 and array_held(g, ref, alt, GRAD_TOL), (keys, opts, name)
    hip_ops.release()


# ---- 3, 4: the exact gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", ["alone", "both"])
def test_exact_gradient(oracle, oracle_nvfma, hip_ops, sides, keys):
    s = sides[keys]
    pb = s.pb
    hip_ops.release()
    s.install(hip_ops)
    m = model(pb)
    out = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact_adjoint=True)
    f, g = float(out[0]), [t.cpu().numpy() for t in out[1:4]]
    assert abs(f - s.f) <= 8 * EPS * s.f
    X.outside_is_zero(pb, g, "exact w2 gradient " + keys)
    w = [{"ett": torch.from_numpy(a).cuda()} for a in s.a]
    jt = [t.cpu().numpy() for t in hip_ops.born_adjoint(*m, w, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])]
    for name, x, y in zip(GRADS, g, jt):
        gap = d64(x, -y) / l2(y)
        print("w2 3 %s %s: exact gradient against -J^T a: rel-L2 %.2e" % (keys, name, gap))
        assert l2(y) > 0 and gap <= 1e-5, (keys, name)
    v = X.smooth_v(pb, 3)
    jv = [G.jv_ett(lib, plain(pb), v) for lib in (oracle, oracle_nvfma)]
    rr, aa = -G.dot(s.a, jv[0]), -G.dot(s.a, jv[1])
    held(X.model_dot(v, g), rr, aa, "w2 4 %s <g, v> = -<a, J v>" % keys, scale=abs(rr))
    hip_ops.release()


# ---- 5: refusals -------------------------------------------------------------------------------------------------------------------------------
def test_products_are_refused(hip_ops, sides):
    from sepfwi import _native
    s = sides["both"]
    pb = s.pb
    hip_ops.release()
    v = X.smooth_v(pb, 3)
    for exact in (False, True):
        with pytest.raises(_native.SepFwiError) as e:
            hip_ops.gauss_newton(*model(pb), *cuda(v), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact=exact)
        assert e.value.code == -1 and W.KEY in str(e.value), (exact, str(e.value))
    x = flat(s.syn).cuda()
    with pytest.raises(_native.SepFwiError) as e:
        hip_ops.data_gn(x, x, pb["Shot_ids"], pb["para_fname"])
    assert e.value.code == -1 and W.KEY in str(e.value)
    d = hip_ops.born(*model(pb), *cuda(v), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])      # the scattered gathers alone are served
    assert all(float(g["ett"].abs().max()) > 0 for g in d)
    hip_ops.release()


BAD = {"if_cross_misfit": True, "if_envelope_misfit": True, "if_src_update": True, "misfit_w_vx": 0.5}
BETAS = {"zero": 0.0, "negative": -1.0, "seventeen": 17.0, "nan": float("nan")}


@pytest.mark.parametrize("other", list(BAD) + ["beta_" + k for k in BETAS])
def test_refusals_reach_the_c_abi(hip_ops, sides, other):
    """the key with each incompatible key: -1 (SEPFWI_EINVAL) and both key names; w2_beta outside (0, 16]: -1 and its name; NaN is no JSON
    number: the reader's error, whatever its code.  Before a session exists; a session of a good file works afterwards."""
    from sepfwi import _native
    L = _native.lib()
    s = sides["alone"]
    hip_ops.release()
    more = {other: BAD[other]} if other in BAD else {W.BETA_KEY: BETAS[other[5:]]}
    bad = w2_problem(s.pb["para_fname"].rsplit("/", 1)[0] + "/bad_" + other, "alone", **more)
    m = model(bad)
    stf, ids = bad["Stf"].contiguous(), np.ascontiguousarray(bad["Shot_ids"].numpy(), dtype=np.int32)
    mis = torch.zeros(1)
    p = lambda t: C.c_void_p(t.data_ptr())
    x = torch.zeros(sum(g.size for g in s.obs))
    rcs = [L.sepfwi_cufd(p(mis), None, None, None, None, *[p(t) for t in m], p(stf), 0, 0, int(ids.size), C.c_void_p(ids.ctypes.data), bad["para_fname"].encode())]
    msgs = [L.sepfwi_last_error()]
    rcs.append(L.sepfwi_data_misfit(p(mis), None, p(x), p(x), 0, int(ids.size), C.c_void_p(ids.ctypes.data), bad["para_fname"].encode(), None))
    msgs.append(L.sepfwi_last_error())
    print("w2 5 %s: %s %s" % (other, rcs, msgs[0]))
    for rc, msg in zip(rcs, msgs):
        if other == "beta_nan":
            assert rc != 0, (rc, msg)
        elif other in BAD:
            assert rc == -1 and W.KEY.encode() in msg and other.encode() in msg, (rc, msg)
        else:
            assert rc == -1 and W.BETA_KEY.encode() in msg, (rc, msg)
    s.install(hip_ops)
    f = float(hip_ops.forward(*model(s.pb), s.pb["Stf"], 0, s.pb["Shot_ids"], s.pb["para_fname"])[0])
    assert abs(f - s.f) <= 8 * EPS * s.f
    hip_ops.release()


# ---- 6: reference mode ---------------------------------------------------------------------------------------------------------------------------
def test_reference_mode_ignores_the_key(hip_ops, sides):
    """"conditioning": "reference" with the key (and a filter): the bits of the plain L2 file."""
    s = sides["filter"]
    here = s.pb["para_fname"].rsplit("/", 1)[0]
    ref_mode = w2_problem(here + "/refmode", "filter", conditioning="reference")
    l2_file = w2_problem(here + "/l2", "alone", key=False)
    hip_ops.release()
    out = []
    for pb in (ref_mode, l2_file):
        s.install(hip_ops, pb)
        out.append(hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"]))
    assert float(out[0][0]) > 0 and all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(*out))
    hip_ops.release()


# ---- 7: untouched -----------------------------------------------------------------------------------------------------------------------------------
def live_bytes():
    from sepfwi import _native
    d, h = C.c_longlong(0), C.c_longlong(0)
    _native.check(_native.lib().sepfwi_debug_live_bytes(C.byref(d), C.byref(h)))
    return d.value, h.value


@pytest.mark.parametrize("keys", ["alone", "both"])
def test_a_file_without_the_key_is_untouched(hip_ops, sides, keys):
    """the same file without the key: launches, device_bytes and output bits of a gradient call before and after a session under the key
    ran a gradient call and the data-space entry point in the same process; under the key the same call costs more launches only where the
    file had no conditioner before; live device bytes return to their start after release."""
    s = sides[keys]
    keyed = s.pb
    unkeyed = w2_problem(keyed["para_fname"].rsplit("/", 1)[0] + "/untouched", keys, key=False)
    hip_ops.release()
    start = live_bytes()

    def run(pb):
        s.install(hip_ops, pb)
        out = hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
        st = hip_ops.stats(pb["para_fname"])
        return out, st["launches"], st["device_bytes"]

    before = run(unkeyed)
    with_key = run(keyed)
    hip_ops.data_misfit(flat(s.obs).cuda(), flat(s.syn).cuda(), keyed["Shot_ids"], keyed["para_fname"])
    after = run(unkeyed)
    print("w2 7 %s: launches of a gradient call without the key %d and %d, under the key %d; device bytes %d, %d, %d" % (keys, before[1], after[1], with_key[1], before[2], after[2], with_key[2]))
    assert before[1] == after[1] and before[2] == after[2], (before[1:], after[1:])
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(before[0], after[0]))
    if keys == "both":      # the file had its conditioner: per shot the residual kernel's one launch becomes the W2 misfit's two
        assert with_key[1] == before[1] + len(G.shots_of(keyed))
    hip_ops.release()
    assert live_bytes() == start
