"""The tangent of the parameter chain on the GPU (-m gpu): k_param_jvp, k_param_diag and k_param_diag_rim of csrc/param_maps.hip through
sepfwi_param_jvp / sepfwi_param_diag and _MaskedTriple.tangent / pullback / diag / born / gauss_newton, PyTorchObjective.hessp and
examples/gauss_newton_fwi.py --param vp_vs_den.

References and bounds, none new (tests/param_tangent_ref.py): the float64 torch.func.jvp of the modules' own expression and its dense
Jacobian, each output array within 2e-6 (algebraic kinds) / 1e-6 (rock physics) of its largest reference entry; the transpose identity
within the Hoelder sum of those; at module level the CPU reference of Born modelling (tests/exact_adjoint_ref.py, tests/born_ref.py) with
the seismogram bound of tests/test_gpu_born.py (1e-4, max-norm and rel-L2) and `held` of tests/test_gpu_exact_adjoint.py
(1e-3 |ref| + 3 |alt - ref| over the two oracle builds).  Every comparison prints its figure before it asserts
(profiles/r19_param_tangent.txt holds those measured on the MI355X).

Every test fails on the parent: the entry points and the methods are missing."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exact_adjoint_ref as X
import param_tangent_ref as T
import problems as P
import pseudo_hessian_ref as R
from conftest import ROOT
from exact_adjoint_ref import held

pytestmark = pytest.mark.gpu

GRIDS = [(3, 5, 2, 1),      # partial blocks in both directions
         (1, 1, 1, 0),      # one physical cell, everything replicates it: the rim kernel's degenerate branches
         (4, 61, 2, 3),     # nxp = 65 crosses the 64-wide block, nzp = 11
         (5, 64, 0, 0)]     # no padding at all
SEIS_TOL = 1e-4             # tests/test_gpu_born.py


def _cuda(arrs):
    return [torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda") for a in arrs]


def _np(ts):
    return [t.detach().cpu().numpy() for t in ts]


def _modules(cls_name, dims, mask=None):
    f, rmask, v, w, h = T.inputs(cls_name, dims)
    mask = rmask if mask is None else mask
    gpu = T.make_module(cls_name, dims, f, mask, device="cuda")
    assert gpu._fusable()
    return gpu, T.make_module(cls_name, dims, f, mask), T.make_module(cls_name, dims, f, mask, dtype=torch.float64), mask, v, w, h


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("cls_name", T.CLASSES)
def test_kernels_against_float64_torch(hip_ops, cls_name, dims):
    """sepfwi_param_jvp against the float64 jvp; sepfwi_param_diag against the dense float64 Jacobian on the two small grids and against the
    torch path of `diag` on the two wide ones."""
    gpu, m32, m64, mask, v, w, h = _modules(cls_name, dims)
    tag = "%s %s" % (cls_name, "x".join(map(str, dims)))
    got = gpu.tangent(*_cuda(v))
    assert all(t.is_cuda and tuple(t.shape) == T.padded_shape(dims) for t in got)
    T.close(_np(got), T.tangent64(m64, v), T.tol_of(cls_name), tag + " kernel tangent")
    d = gpu.diag(*_cuda(h))
    assert all(t.is_cuda and tuple(t.shape) == dims[:2] for t in d)
    if dims[1] <= 5:
        T.close(_np(d), T.diag64(m64, h), T.tol_of(cls_name), tag + " kernel diag against the dense Jacobian")
    else:
        T.close(_np(d), _np(m32.diag(*[torch.tensor(a) for a in h])), T.tol_of(cls_name), tag + " kernel diag against the torch path")


@pytest.mark.parametrize("dims", [GRIDS[0], GRIDS[2]], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("cls_name", T.CLASSES)
def test_exactness_properties(hip_ops, cls_name, dims):
    """Asserted with ==: NULL tangents are zero arrays; 0 wherever Mask is 0; linear under a factor 2 (a stray non-linear term, or a
    term that does not carry the tangent, breaks it); a spike at rim cell (0, 0) lands on exactly the corner rectangle times the Mask."""
    gpu, m32, m64, mask, v, w, h = _modules(cls_name, dims)
    nz, nx, nPml, nPad = dims
    vc = _cuda(v)
    zero = torch.zeros_like(vc[0])
    full = _np(gpu.tangent(*vc))
    for keep in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 0, 0)):
        a = _np(gpu.tangent(*[t if k else None for t, k in zip(vc, keep)]))
        b = _np(gpu.tangent(*[t if k else zero for t, k in zip(vc, keep)]))
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), keep
    assert not any(np.any(x) for x in a)                                     # v = 0
    assert (mask == 0).any() and all(np.isfinite(x).all() and not np.any(x[mask == 0]) for x in full)
    twice = _np(gpu.tangent(*[2.0 * t for t in vc]))
    assert all(np.array_equal(x, 2.0 * y) for x, y in zip(twice, full)) and any(np.any(y) for y in full)
    spike = [np.zeros((nz, nx), np.float32) for _ in range(3)]
    for k in range(3):
        spike[k][0, 0] = v[k][0, 0] if v[k][0, 0] != 0 else 1.0
    hit = np.zeros(T.padded_shape(dims), bool)
    for x in _np(gpu.tangent(*_cuda(spike))):
        hit |= x != 0
    corner = np.zeros_like(hit)
    corner[:nPml + 1, :nPml + 1] = True
    assert np.array_equal(hit, corner & (mask != 0))


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_kind_1_is_the_masked_padding(hip_ops, dims):
    """(Lambda, Mu, Den) themselves: P = diag(Mask) E, bit for bit."""
    from sepfwi import utils as ft
    gpu, m32, m64, mask, v, w, h = _modules("FWI_Lame_Den", dims)
    got = _np(gpu.tangent(*_cuda(v)))
    for g, a in zip(got, v):
        assert np.array_equal(g, mask * ft.padding_numpy_array(a, dims[2], dims[3]))


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("cls_name", T.CLASSES)
def test_transpose_identity_against_the_shipped_backward(hip_ops, cls_name, dims):
    """<P v, w> = <v, P^T w> with P^T the shipped sepfwi_param_backward (`pullback` on HIP tensors), dots in float64."""
    gpu, m32, m64, mask, v, w, h = _modules(cls_name, dims)
    Pv, Ptw = _np(gpu.tangent(*_cuda(v))), _np(gpu.pullback(*_cuda(w)))
    lhs, rhs = T.dot(Pv, w), T.dot(v, Ptw)
    bound = T.holder_bound(T.tol_of(cls_name), Pv, w, Ptw, v)
    print("param tangent %s %r transpose identity on the GPU: <P v, w> %.10e, <v, P^T w> %.10e, difference %.2e, bound %.2e"
          % (cls_name, dims, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs) > 0 and abs(lhs - rhs) <= bound


# ---- module level: PROBLEM_A (50 x 90, two shots) as tests/test_gpu_exact_adjoint.py uses it ----------------------------------------
def _rock_fields(shape):
    rng = np.random.default_rng(5)
    return [P.smooth_random(rng, shape, lo, hi).astype(np.float32) for lo, hi in ((0.10, 0.30), (0.05, 0.45), (0.2, 0.9))]


def _direction(f, seed, smooth):
    rng = np.random.default_rng(seed)
    draw = (lambda s: P.smooth_random(rng, s, -1.0, 1.0, passes=6)) if smooth else (lambda s: rng.uniform(-1.0, 1.0, s))
    return [(0.01 * a * draw(a.shape)).astype(np.float32) for a in f]


@pytest.fixture(scope="module", params=["FWI", "FWI_Rock_Physics_gassmann"])
def prob(request, oracle, oracle_nvfma, hip_ops, tmp_path_factory):
    """The module on HIP tensors with Mask = 1 on Omega and 0 elsewhere, a smooth and a white-noise direction in its own parameters,
    P_ref v of each (float64 torch tangent rounded to float32) and J P_ref v on both oracle builds: computed once, left unchanged."""
    from sepfwi import modules as M
    cls_name = request.param
    pb = P.make_problem(str(tmp_path_factory.mktemp("tangent_" + cls_name)), **R.PROBLEM_A)
    dims = (pb["opt"]["nz"], pb["opt"]["nx"], pb["nPml"], pb["nPad"])
    f = [pb["init"][k] for k in ("vp", "vs", "rho")] if cls_name == "FWI" else _rock_fields(dims[:2])
    mask = X.mask_omega(pb).astype(np.float32)
    build = lambda dtype, dev, grads=(True, True, True): getattr(M, cls_name)(
        *[torch.tensor(a, dtype=dtype, device=dev, requires_grad=g) for a, g in zip(f, grads)], pb["Stf"], pb["opt"],
        Mask=torch.tensor(mask, dtype=dtype, device=dev))
    mod, m64 = build(torch.float32, "cuda"), build(torch.float64, "cpu")
    assert mod._fusable()
    pb = dict(pb, lame_mod=tuple(t.cpu() for t in mod._model()))
    vs = [_direction(f, 3, True), _direction(f, 5, False)]
    Pv = [[a.astype(np.float32) for a in T.tangent64(m64, v)] for v in vs]
    ref = [X.jv_ref(oracle, pb, p, model="lame_mod") for p in Pv]
    alt = [X.jv_ref(oracle_nvfma, pb, p, model="lame_mod") for p in Pv]
    return dict(cls=cls_name, pb=pb, mod=mod, build=build, vs=vs, ref=ref, alt=alt)


def _ett(out):
    return {"ett": np.stack([d["ett"].cpu().numpy() for d in out])}


def test_module_born_is_j_p_v(hip_ops, prob):
    """(a) module.born(v) is fwi_ops.born of the hand-composed tangent, bit for bit, and J P_ref v of the CPU reference to the seismogram
    bound."""
    pb, mod = prob["pb"], prob["mod"]
    for k, name in enumerate(("smooth", "white noise")):
        v = _cuda(prob["vs"][k])
        got = _ett(mod.born(v, pb["Shot_ids"]))
        hand = _ett(hip_ops.born(*mod._model(), *mod.tangent(*v), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], ("ett",)))
        assert np.array_equal(got["ett"], hand["ett"])
        w = np.asarray(prob["ref"][k]["ett"], np.float64)
        dmax, l2 = np.abs(got["ett"] - w).max() / np.abs(w).max(), P.rel_l2(got["ett"], w)
        print("param tangent %s module.born, %s v: max-norm deviation %.2e of the maximum, rel-L2 %.2e" % (prob["cls"], name, dmax, l2))
        assert np.abs(w).max() > 0 and dmax <= SEIS_TOL and l2 <= SEIS_TOL


def test_module_gauss_newton_exact_is_symmetric_and_the_norm_of_j_p_v(hip_ops, prob):
    """(b) exact=True: v^T H_p v = |J P v|^2 against the CPU reference and against the GPU's own module.born(v);
    <u, H_p v> = <H_p u, v>."""
    pb, mod, ref, alt = prob["pb"], prob["mod"], prob["ref"], prob["alt"]
    hv = [_np(mod.gauss_newton(_cuda(v), pb["Shot_ids"], exact=True)) for v in prob["vs"]]
    vhv = [X.model_dot(v, h) for v, h in zip(prob["vs"], hv)]
    for k, name in enumerate(("smooth", "white noise")):
        assert all(h.shape == v.shape and np.isfinite(h).all() for h, v in zip(hv[k], prob["vs"][k]))
        held(vhv[k], X.data_dot(ref[k], ref[k]), X.data_dot(alt[k], alt[k]), "%s v^T H_p v, %s" % (prob["cls"], name))
        own = _ett(mod.born(_cuda(prob["vs"][k]), pb["Shot_ids"]))
        n_own = X.data_dot(own, own)
        held(vhv[k], n_own, n_own, "%s v^T H_p v against the GPU's own module.born, %s" % (prob["cls"], name))
    scale = float(np.sqrt(vhv[0] * vhv[1]))
    c21, c12 = X.model_dot(prob["vs"][1], hv[0]), X.model_dot(prob["vs"][0], hv[1])
    cr, ca = X.data_dot(ref[0], ref[1]), X.data_dot(alt[0], alt[1])
    held(c21, c12, c12 + (ca - cr), "%s symmetry <u, H_p v> against <H_p u, v>" % prob["cls"], scale=scale)
    held(c21, cr, ca, "%s <u, H_p v> against <J P u, J P v>" % prob["cls"], scale=scale)


@pytest.mark.parametrize("exact", [True, False])
def test_module_gauss_newton_is_the_hand_composition(hip_ops, prob, exact):
    """(c), (e): pullback(fwi_ops.gauss_newton(tangent(v))), for the exact adjoint and for sepfwi_born's product.  Equality where two
    identical fwi_ops.gauss_newton calls agree bit for bit; otherwise 3 x their difference."""
    pb, mod = prob["pb"], prob["mod"]
    v = _cuda(prob["vs"][0])
    raw = lambda: hip_ops.gauss_newton(*mod._model(), *mod.tangent(*v), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact=exact)
    r1, r2 = raw(), raw()
    got = _np(mod.gauss_newton(v, pb["Shot_ids"], exact=exact))
    hand = _np(mod.pullback(*r1))
    assert all(np.abs(h).max() > 0 for h in hand)
    if all(torch.equal(a, b) for a, b in zip(r1, r2)):
        assert all(np.array_equal(a, b) for a, b in zip(got, hand))
    else:
        again = _np(mod.pullback(*r2))
        for a, b, c in zip(got, hand, again):
            run = np.abs(b - c).max()
            print("param tangent %s gauss_newton(exact=%r): run-to-run difference %.2e, module against hand composition %.2e" % (prob["cls"], exact, run, np.abs(a - b).max()))
            assert np.abs(a - b).max() <= 3.0 * run


def test_only_the_middle_field_inverted(hip_ops, prob):
    """(d) a module where only the second field requires grad: None entries of v, and hessp on it."""
    from sepfwi.obj_wrapper import PyTorchObjective
    pb, full = prob["pb"], prob["mod"]
    part = prob["build"](torch.float32, "cuda", (False, True, False))
    name = part.NAMES[1]
    assert part._fusable() and [n for n, _ in part.named_parameters()] == [name]
    dv = _cuda(prob["vs"][0])[1]
    zero = torch.zeros_like(dv)
    a, b = part.tangent(None, dv, None), full.tangent(zero, dv, zero)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    want = _np(full.gauss_newton((zero, dv, zero), pb["Shot_ids"], exact=True))[1]
    got = _np(part.gauss_newton((None, dv, None), pb["Shot_ids"], exact=True))
    assert len(got) == 3 and np.abs(want).max() > 0
    obj = PyTorchObjective(part, lambda: part(pb["Shot_ids"], ngpu=1), shot_ids=pb["Shot_ids"], exact=True)
    hp = obj.hessp(obj.x0, prob["vs"][0][1].ravel().astype(np.float64))
    assert hp.dtype == np.float64 and hp.shape == (dv.numel(),)
    run = np.abs(want - _np(full.gauss_newton((zero, dv, zero), pb["Shot_ids"], exact=True))[1]).max()      # run to run
    for x, what in ((got[1], "gauss_newton with None entries"), (hp.reshape(want.shape), "hessp")):
        dev = np.abs(x - want).max()
        print("param tangent %s %s against the middle block of the full product: %.2e (run to run %.2e)" % (prob["cls"], what, dev, run))
        assert dev <= 3.0 * run


def test_trust_ncg_with_hessp(tmp_path, hip_ops):
    """scipy.optimize.minimize(method="trust-ncg") over PyTorchObjective.hessp: the FWI module on HIP tensors, exact=True.  Every curvature
    p^T H p the solver sees is non-negative and the misfit ends below where it started."""
    from scipy import optimize
    from sepfwi import modules as M
    from sepfwi.obj_wrapper import PyTorchObjective
    pb = P.make_problem(str(tmp_path))
    hip_ops.obscalc(*pb["lame_true"], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    f = [torch.tensor(pb["init"][k], device="cuda", requires_grad=True) for k in ("vp", "vs", "rho")]
    fwi = M.FWI(f[0], f[1], f[2], pb["Stf"], pb["opt"])
    obj = PyTorchObjective(fwi, lambda: fwi(pb["Shot_ids"], ngpu=1), shot_ids=pb["Shot_ids"], exact=True)
    curv = []

    def hessp(x, p):
        hp = obj.hessp(x, p)
        curv.append(float(p @ hp))
        return hp

    fun, jac = obj.fun, obj.jac      # (bound before the first evaluation: cache() stores the gradient under the name `jac`, as the reference's glue does)
    f_start = fun(obj.x0)
    res = optimize.minimize(fun, obj.x0, jac=jac, hessp=hessp, method="trust-ncg", options={"maxiter": 3})
    print("param tangent trust-ncg: misfit %.8e -> %.8e in %d iterations, %d products, smallest p^T H p %.3e" % (f_start, res.fun, res.nit, len(curv), min(curv)))
    assert curv and min(curv) >= 0.0
    assert res.fun < f_start


def test_example_in_vp_vs_den_reduces_the_misfit(tmp_path):
    """examples/gauss_newton_fwi.py --param vp_vs_den, as tests/test_gpu_born_example.py runs the default parameterisation."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "gauss_newton_fwi.py"), "--device", "cuda", "--param", "vp_vs_den",
                          "--exact-adjoint", "--outer", "2", "--inner", "3", "--nsteps", "700", "--shot-stride", "3", "--rtol", "1e-6",
                          "--workdir", str(tmp_path)], capture_output=True, text=True, timeout=300, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    lines = out.stdout.splitlines()
    f = [float(ln.split("misfit")[1].split()[0]) for ln in lines if ln.startswith("iterate ") and "misfit" in ln]
    assert len(f) == 3 and f[1] < f[0] and f[2] < f[1], out.stdout[-2000:]
    for k in (1, 2):
        r = [float(ln.split("residual")[1]) for ln in lines if ln.startswith("  outer %d cg" % k)]
        assert len(r) == 3 and r[-1] < 1.0 and r[-1] < r[0], (k, r)
    assert any(ln.startswith("done: ") for ln in lines) and any(ln.lstrip().startswith("Vp ") for ln in lines)
