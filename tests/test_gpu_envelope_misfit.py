"""The envelope misfit through the passes, on the GPU (-m gpu): parameter key if_envelope_misfit under sepfwi_cufd (calc_id 0 and 1, stream
and batched schedule, bwd_fuse), sepfwi_adjoint_exact (gradient and product), sepfwi_born with hv_*, obj_wrapper.gauss_newton_cg, the
refusals, and what a file without the key keeps.  The yardstick is outside the GPU (tests/envelope_ref.py, licensed by
tests/test_envelope_reference.py): H, e, D, D^T in numpy float64; C and C^T the oracle's; gradients of the reference-style pass from
oracle.cufd(calc_id 1, adj_src = a); J from tests/born_ref.py.

Problem: problems.cond_problem's sizes (44 x 60, 300 steps, two shots, its windows and weights) under the key alone, with filter, with
if_win, with both (envelope_ref.gpu_problem).  Tolerances, none new:
  misfit        the suite's 1e-4 (+ 3 x the two oracle builds' difference)
  gradients     rel-L2 1e-3 + 3 |g_ref - g_ref_nvfma|, the two-oracle-build yardstick of tests/fuzz_common.py; gStf likewise
  exact passes  tests/exact_adjoint_ref.py: held -- 1e-3 of the scale + 3 x the builds' difference
Every comparison prints its deviation before it asserts; profiles/r21_envelope_misfit.txt holds the figures measured on the MI355X and what
six deliberately wrong variants of the pass do to them.

On the parent commit the key is ignored and the L2 misfit comes back: every comparison against the reference fails there (the inputs differ
from the L2 ones by far more than the tolerances: tests/test_envelope_reference.py::test_inputs_of_the_gpu_tests_discriminate)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cond_gn_ref as G
import envelope_ref as E
import exact_adjoint_ref as X
import problems as P
import stf_ref as S
from exact_adjoint_ref import cuda, held
from fuzz_common import GRAD_TOL, MISFIT_TOL, array_held, d64, l2, scalar_held
from sepfwi import utils as ft

pytestmark = pytest.mark.gpu
GRADS = ("gLambda", "gMu", "gDen")
OPTIONS = {"default": dict(), "stream": dict(batch=0), "two_launch": dict(bwd_fuse=2)}


def model(pb, which="lame_init"):
    return [t.cuda() for t in pb[which]]


def flat(gathers):
    return torch.from_numpy(np.concatenate([np.asarray(g, np.float32).reshape(-1) for g in gathers]))


class Side:
    """one key set: the problem and, on both oracle builds, the raw gathers of lame_true (obs) and lame_init (syn), the reference misfit,
    adjoint source and reference-style gradient"""

    def __init__(self, libs, tmp, keys):
        self.keys, self.libs = keys, libs
        self.pb = pb = E.gpu_problem(tmp, keys)
        self.obs, self.syn, self.misfit, self.adj, self.grad = [], [], [], [], []
        for lib in libs:
            obs, _ = G.oracle_gathers(lib, pb, "lame_true")
            syn, _ = G.oracle_gathers(lib, pb, "lame_init")
            f, a, _, _ = E.data_misfit(lib, pb, obs, syn)
            self.obs.append(obs)
            self.syn.append(syn)
            self.misfit.append(f)
            self.adj.append(a)
            self.grad.append(E.gradient(lib, pb, a))

    def install(self, hip_ops, pb=None):
        """the first build's observed gathers into the session of pb (raw: the session conditions them)"""
        pb = pb or self.pb
        for i, sid in enumerate(G.shots_of(pb)):
            hip_ops.set_observed(pb["para_fname"], sid, torch.from_numpy(np.ascontiguousarray(self.obs[0][i])))


@pytest.fixture(scope="module")
def sides(oracle, oracle_nvfma, tmp_path_factory):
    """computed once, left unchanged"""
    return {k: Side((oracle, oracle_nvfma), tmp_path_factory.mktemp("env_" + k), k) for k in E.KEYSETS}


@pytest.fixture(scope="module")
def vside(sides):
    """two smooth v on Omega, a source perturbation each, and J v (+ J_s ds) on both builds, for the key sets the exact tests run"""
    pb = sides["both"].pb
    vs = [X.smooth_v(pb, s) for s in (3, 4)]
    ds = [S.draw_ds(k, pb["Stf"].numpy(), S.DS_SCALE) for k in range(2)]
    plain = dict(pb, para=E.plain_para(pb))
    jv = [[G.jv_ett(lib, plain, v) for v in vs] for lib in sides["both"].libs]
    ju = [[G.jv_ett(lib, plain, v, d) for v, d in zip(vs, ds)] for lib in sides["both"].libs]
    js = [G.jv_ett(lib, plain, None, ds[0]) for lib in sides["both"].libs]
    return dict(vs=vs, ds=ds, jv=jv, ju=ju, js=js)


# ---- 1: misfit and gradient against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", list(OPTIONS))
@pytest.mark.parametrize("keys", list(E.KEYSETS))
def test_misfit_and_gradient_against_the_reference(hip_ops, sides, keys, opts):
    s = sides[keys]
    pb = s.pb
    hip_ops.release()
    with P.kernel_options(**OPTIONS[opts]):
        s.install(hip_ops)
        out = hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    f = float(out[0])
    print("envelope 1 %s %s: misfit %.8e, reference %.8e (relative gap %.2e; the two oracle builds %.2e)"
          % (keys, opts, f, s.misfit[0], abs(f - s.misfit[0]) / s.misfit[0], abs(s.misfit[1] - s.misfit[0]) / s.misfit[0]))
    assert scalar_held(f, s.misfit[0], s.misfit[1], MISFIT_TOL)
    got = dict(zip(GRADS + ("gStf",), [t.cpu().numpy() for t in out[1:5]]))
    for name in GRADS + ("gStf",):
        ref, alt = s.grad[0][name], s.grad[1][name]
        g = got[name][:ref.shape[0]] if name == "gStf" else got[name]
        print("envelope 1 %s %s %s: rel-L2 %.2e (the two oracle builds %.2e)" % (keys, opts, name, d64(g, ref) / l2(ref), d64(alt, ref) / l2(ref)))
        assert l2(ref) > 0 and array_held(g, ref, alt, GRAD_TOL), (keys, opts, name)
    hip_ops.release()


# ---- 2: entry points --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", ["alone", "both"])
def test_entry_points_agree(hip_ops, sides, keys):
    """forward (calc_id 0) gives the misfit of backward to 1e-6; observed data set from memory give the bits of the files; the misfit
    equals data_misfit of the oracle's gathers to 1e-4."""
    s = sides[keys]
    pb = s.pb
    hip_ops.release()
    m = model(pb)
    hip_ops.obscalc(*model(pb, "lame_true"), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])      # the four files per shot
    from_files = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    f0 = float(hip_ops.forward(*m, pb["Stf"], 0, pb["Shot_ids"], pb["para_fname"])[0])
    f1 = float(from_files[0])
    print("envelope 2 %s: forward %.8e, backward %.8e (relative gap %.2e)" % (keys, f0, f1, abs(f0 - f1) / f1))
    assert f1 > 0 and abs(f0 - f1) <= 1e-6 * f1
    hip_ops.release()
    for sid in G.shots_of(pb):
        hip_ops.set_observed(pb["para_fname"], sid, torch.from_numpy(ft.read_shot_gather(pb["data_dir"], "ett", sid, pb["nSteps"])))
    from_memory = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(from_files, from_memory))
    hip_ops.release()
    s.install(hip_ops)
    f = float(hip_ops.forward(*m, pb["Stf"], 0, pb["Shot_ids"], pb["para_fname"])[0])
    fd, _ = hip_ops.data_misfit(flat(s.obs[0]).cuda(), flat(s.syn[0]).cuda(), pb["Shot_ids"], pb["para_fname"])
    print("envelope 2 %s: misfit call %.8e, data_misfit of the oracle's gathers %.8e (relative gap %.2e)" % (keys, f, fd, abs(f - fd) / fd))
    assert abs(f - fd) <= MISFIT_TOL * fd
    hip_ops.release()


# ---- 3: the exact gradient ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", ["alone", "both"])
def test_exact_gradient(hip_ops, sides, vside, keys):
    """backward(exact_adjoint=True, source_gradient=True): <g, P v> = -<a, J P v> and <g_stf, ds> = -<a, J_s ds>, a the reference's
    raw-space adjoint source; the misfit is a misfit call's."""
    s = sides[keys]
    pb = s.pb
    hip_ops.release()
    s.install(hip_ops)
    m = model(pb)
    f0 = float(hip_ops.forward(*m, pb["Stf"], 0, pb["Shot_ids"], pb["para_fname"])[0])
    out = hip_ops.backward(*m, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact_adjoint=True, source_gradient=True)
    f = float(out[0])
    print("envelope 3 %s: misfit of the exact pass %.8e, of a misfit call %.8e, of the reference %.8e" % (keys, f, f0, s.misfit[0]))
    assert abs(f - f0) <= MISFIT_TOL * f0 and scalar_held(f, s.misfit[0], s.misfit[1], MISFIT_TOL)
    g = [t.cpu().numpy() for t in out[1:4]]
    X.outside_is_zero(pb, g, "exact envelope gradient " + keys)
    for k, v in enumerate(vside["vs"]):
        rr, aa = -G.dot(s.adj[0], vside["jv"][0][k]), -G.dot(s.adj[1], vside["jv"][1][k])
        held(X.model_dot(v, g), rr, aa, "envelope 3 %s <g, v>, v %d" % (keys, k), scale=abs(rr))
    gs = out[4].numpy()
    assert gs.shape == tuple(pb["Stf"].shape) and np.abs(gs).max() > 0
    rr, aa = -G.dot(s.adj[0], vside["js"][0]), -G.dot(s.adj[1], vside["js"][1])
    held(S.stf_dot(vside["ds"][0], gs), rr, aa, "envelope 3 %s <g_stf, ds>" % keys, scale=abs(rr))
    hip_ops.release()


# ---- 4: the products --------------------------------------------------------------------------------------------------------------------------------
def gn(hip_ops, pb, v, exact=True, dStf=None):
    out = hip_ops.gauss_newton(*model(pb), *(cuda(v) if v is not None else (None, None, None)), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact=exact,
                               dStf=None if dStf is None else torch.from_numpy(dStf))
    return [h.cpu().numpy() for h in out]


@pytest.mark.parametrize("keys", ["alone", "both"])
def test_exact_product(hip_ops, sides, vside, keys):
    """gauss_newton(exact=True): v^T H v = |Z D C J P v|^2, u^T H v = v^T H u = <Z D C J u, Z D C J v>, D at C of the background gather;
    with dStf the same with the fourth block."""
    s = sides[keys]
    pb, vs, ds = s.pb, vside["vs"], vside["ds"]
    hip_ops.release()
    for what, jside, with_ds in (("v", vside["jv"], False), ("[v; ds]", vside["ju"], True)):
        z = [[E.zdc(lib, pb, s.syn[b], jside[b][k]) for k in range(2)] for b, lib in enumerate(s.libs)]
        hv = [gn(hip_ops, pb, v, dStf=d if with_ds else None) for v, d in zip(vs, ds)]
        udot = lambda k, o: X.model_dot(vs[k], o[:3]) + (S.stf_dot(ds[k], o[3]) if with_ds else 0.0)
        uhu = [udot(k, hv[k]) for k in range(2)]
        for k in range(2):
            X.outside_is_zero(pb, hv[k][:3], keys)
            assert len(hv[k]) == (4 if with_ds else 3)
            held(uhu[k], G.dot(z[0][k], z[0][k]), G.dot(z[1][k], z[1][k]), "envelope 4 %s %s^T H %s, %d" % (keys, what, what, k))
        scale = float(np.sqrt(uhu[0] * uhu[1]))
        c21, c12 = udot(1, hv[0]), udot(0, hv[1])
        cr, ca = G.dot(z[0][0], z[0][1]), G.dot(z[1][0], z[1][1])
        held(c21, c12, c12 + (ca - cr), "envelope 4 %s %s symmetry" % (keys, what), scale=scale)
        held(c21, cr, ca, "envelope 4 %s %s cross term against the reference" % (keys, what), scale=scale)
    hip_ops.release()


@pytest.mark.parametrize("keys", ["alone", "both"])
def test_reference_style_product_and_raw_born_gathers(hip_ops, sides, vside, keys):
    """gauss_newton(exact=False) against oracle.cufd(adj_src = -C^T D^T Z D C J v) with J v from born_ref, to 1e-3 |g| + 3 |g - g_nvfma|;
    the Born gathers handed out under the key are bit for bit those of the same file without it."""
    s = sides[keys]
    pb, v = s.pb, vside["vs"][0]
    hip_ops.release()
    hv = gn(hip_ops, pb, v, exact=False)
    ref = [E.gradient(lib, pb, [-x for x in E.data_gn(lib, pb, s.syn[b], vside["jv"][b][0])]) for b, lib in enumerate(s.libs)]
    for name, got in zip(GRADS, hv):
        r, a = ref[0][name], ref[1][name]
        print("envelope 4 %s reference-style product %s: rel-L2 %.2e (the two oracle builds %.2e)" % (keys, name, d64(got, r) / l2(r), d64(a, r) / l2(r)))
        assert l2(r) > 0 and array_held(got, r, a, GRAD_TOL), (keys, name)
    plain = E.gpu_problem(pb["para_fname"].rsplit("/", 1)[0] + "/plain", keys, key=False)
    raw = lambda q: [d["ett"].cpu().numpy() for d in hip_ops.born(*model(pb), *cuda(v), pb["Stf"], 1, pb["Shot_ids"], q["para_fname"])]
    a, b = raw(pb), raw(plain)
    assert all(np.abs(x).max() > 0 and np.array_equal(x, y) for x, y in zip(a, b))
    hip_ops.release()


# ---- 5: conjugate gradients on the product ------------------------------------------------------------------------------------------------------
def test_gauss_newton_cg_under_the_key(hip_ops, sides):
    """three inner iterations of obj_wrapper.gauss_newton_cg on the exact product: it completes, and the quadratic model
    q(p) = <g, p> + 1/2 <p, H p> decreases monotonically over the iterates."""
    from sepfwi.obj_wrapper import gauss_newton_cg
    s = sides["both"]
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
    print("envelope 5: quadratic model over three conjugate-gradient iterations %s, residual history %s" % (["%.6e" % x for x in q], ["%.3e" % h for h in hist]))
    assert all(b < a for a, b in zip(q[:-1], q[1:])), q
    hip_ops.release()


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", ["if_cross_misfit", "if_src_update", "misfit_w_vx"])
def test_refusals_reach_the_c_abi(hip_ops, sides, other):
    """the key with if_cross_misfit, with if_src_update, with joint weights: -1 (SEPFWI_EINVAL) and both key names at the C ABI, before a
    session exists; a session of a good file works afterwards."""
    from sepfwi import _native
    L = _native.lib()
    s = sides["alone"]
    hip_ops.release()
    bad = E.gpu_problem(s.pb["para_fname"].rsplit("/", 1)[0] + "/bad_" + other, "alone", **{other: 0.5 if other == "misfit_w_vx" else True})
    m = model(bad)
    stf, ids = bad["Stf"].contiguous(), np.ascontiguousarray(bad["Shot_ids"].numpy(), dtype=np.int32)
    mis = torch.zeros(1)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = L.sepfwi_cufd(p(mis), None, None, None, None, *[p(t) for t in m], p(stf), 0, 0, int(ids.size), C.c_void_p(ids.ctypes.data), bad["para_fname"].encode())
    msg = L.sepfwi_last_error()
    assert rc == -1 and E.KEY.encode() in msg and other.encode() in msg, (rc, msg)
    x = torch.zeros(sum(g.size for g in s.obs[0]))
    rc = L.sepfwi_data_misfit(p(mis), None, p(x), p(x), 0, int(ids.size), C.c_void_p(ids.ctypes.data), bad["para_fname"].encode(), None)
    assert rc == -1 and E.KEY.encode() in L.sepfwi_last_error() and other.encode() in L.sepfwi_last_error()
    s.install(hip_ops)
    f = float(hip_ops.forward(*model(s.pb), s.pb["Stf"], 0, s.pb["Shot_ids"], s.pb["para_fname"])[0])
    assert scalar_held(f, s.misfit[0], s.misfit[1], MISFIT_TOL)
    hip_ops.release()


def test_reference_mode_ignores_the_key(hip_ops, sides):
    """"conditioning": "reference" with the key (and a filter): the bits of the plain L2 file."""
    s = sides["filter"]
    here = s.pb["para_fname"].rsplit("/", 1)[0]
    ref_mode = E.gpu_problem(here + "/refmode", "filter", conditioning="reference")
    plain = E.gpu_problem(here + "/l2", "alone", key=False)
    hip_ops.release()
    out = []
    for pb in (ref_mode, plain):
        s.install(hip_ops, pb)
        out.append(hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"]))
    assert float(out[0][0]) > 0 and all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(*out))
    hip_ops.release()


# ---- 7: untouched ---------------------------------------------------------------------------------------------------------------------------------------
def live_bytes():
    from sepfwi import _native
    d, h = C.c_longlong(0), C.c_longlong(0)
    _native.check(_native.lib().sepfwi_debug_live_bytes(C.byref(d), C.byref(h)))
    return d.value, h.value


@pytest.mark.parametrize("keys", ["alone", "both"])
def test_a_file_without_the_key_is_untouched(hip_ops, sides, vside, keys):
    """the same file without the key: launches, device_bytes and output bits of a gradient call before and after a session under the key
    ran a gradient call, a product and the data-space entry points in the same process; live device bytes return to their start after
    release."""
    s = sides[keys]
    keyed = s.pb
    plain = E.gpu_problem(keyed["para_fname"].rsplit("/", 1)[0] + "/untouched", keys, key=False)
    hip_ops.release()
    start = live_bytes()

    def run_plain():
        s.install(hip_ops, plain)
        out = hip_ops.backward(*model(plain), plain["Stf"], 1, plain["Shot_ids"], plain["para_fname"])
        st = hip_ops.stats(plain["para_fname"])
        return out, st["launches"], st["device_bytes"]

    before = run_plain()
    s.install(hip_ops)
    hip_ops.backward(*model(keyed), keyed["Stf"], 1, keyed["Shot_ids"], keyed["para_fname"])
    gn(hip_ops, keyed, vside["vs"][0])
    hip_ops.data_gn(flat(s.syn[0]).cuda(), flat(s.obs[0]).cuda(), keyed["Shot_ids"], keyed["para_fname"])
    after = run_plain()
    assert before[1] == after[1] and before[2] == after[2], (before[1:], after[1:])
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(before[0], after[0]))
    hip_ops.release()
    assert live_bytes() == start
