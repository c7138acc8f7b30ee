"""The tangent of the parameter chain without a GPU: the two C-ABI entry points (sepfwi_param_jvp, sepfwi_param_diag) are exported,
declared and validate their sizes before they touch a device; the torch path of _MaskedTriple.tangent / pullback / diag on CPU tensors
against float64 references (tests/param_tangent_ref.py); PyTorchObjective.hessp on a stand-in module.

Measured here (float32 torch path against the float64 jvp of the same expression, grid (3, 5, 2, 1), v = 1 % noise, largest over the
arrays): tangent 1.4e-7 (algebraic kinds), 3.7e-7 (Voigt-Reuss-Hill), 2.5e-7 (Biot-Gassmann); diag 1.6e-7 / 3.7e-7 / 2.1e-7; transpose
identity at most 1.1e-2 of its Hoelder bound (profiles/r19_param_tangent.txt, which also says how the inputs' seed was chosen)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import param_tangent_ref as T
from conftest import ROOT


def test_symbols_are_exported_declared_and_validate_without_a_device(tmp_path):
    from sepfwi import _native
    L = _native.lib()
    for name in ("sepfwi_param_jvp", "sepfwi_param_diag"):
        assert name in _native.EXPORTS
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == 19
    inc = os.path.join(ROOT, "include")
    body = ('#include "sepfwi.h"\nint call(const float *p, float *q) {\n'
            '    return sepfwi_param_jvp(0, 1, 1, 0, 0, p, p, p, p, p, p, p, p, 0, 0, q, q, q, 0)\n'
            '         + sepfwi_param_diag(0, 1, 1, 0, 0, p, p, p, p, p, p, p, p, p, p, q, q, q, 0);\n}\n')
    (tmp_path / "t.c").write_text(body)
    (tmp_path / "t.cpp").write_text(body)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", inc, str(tmp_path / "t.c")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", inc, str(tmp_path / "t.cpp")])
    for f in (L.sepfwi_param_jvp, L.sepfwi_param_diag):
        for kind, nz, nPml in ((7, 3, 2), (0, 0, 2), (0, 3, -1)):      # NULL arrays: refused before any pointer is looked at
            assert f(kind, nz, 5, nPml, 1, *([None] * 13), None) == -1      # SEPFWI_EINVAL
            assert b"param maps" in L.sepfwi_last_error()


def _pair(cls_name, mask=None):
    f, rmask, v, w, h = T.inputs(cls_name, T.SMALL)
    mask = rmask if mask is None else mask
    m32 = T.make_module(cls_name, T.SMALL, f, mask)
    m64 = T.make_module(cls_name, T.SMALL, f, mask, dtype=torch.float64)
    assert not m32._fusable()
    return v, w, h, m32, m64


@pytest.mark.parametrize("cls_name", T.CLASSES)
def test_torch_tangent_against_the_float64_jvp(cls_name):
    v, w, h, m32, m64 = _pair(cls_name)
    got = m32.tangent(*[torch.tensor(a) for a in v])
    assert all(t.dtype == torch.float32 and tuple(t.shape) == T.padded_shape(T.SMALL) for t in got)
    ref = T.tangent64(m64, v)
    T.close([t.numpy() for t in got], ref, T.tol_of(cls_name), cls_name + " torch tangent")
    # None = a field that is not perturbed
    part = m32.tangent(None, torch.tensor(v[1]), None)
    zeros = m32.tangent(torch.zeros(T.SMALL[:2]), torch.tensor(v[1]), torch.zeros(T.SMALL[:2]))
    assert all(torch.equal(a, b) for a, b in zip(part, zeros))
    assert any(float(t.abs().max()) > 0 for t in part)
    with pytest.raises(ValueError):
        m32.tangent(torch.zeros(2, 2), None, None)


@pytest.mark.parametrize("cls_name", T.CLASSES)
def test_pullback_is_the_transpose_of_tangent(cls_name):
    v, w, h, m32, m64 = _pair(cls_name)
    Pv = [t.numpy() for t in m32.tangent(*[torch.tensor(a) for a in v])]
    Ptw = [t.numpy() for t in m32.pullback(*[torch.tensor(a) for a in w])]
    assert all(a.shape == T.SMALL[:2] for a in Ptw)
    lhs, rhs = T.dot(Pv, w), T.dot(v, Ptw)
    bound = T.holder_bound(T.tol_of(cls_name), Pv, w, Ptw, v)
    print("param tangent %s transpose identity: <P v, w> %.10e, <v, P^T w> %.10e, difference %.2e, bound %.2e" % (cls_name, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs) > 0 and abs(lhs - rhs) <= bound
    # a None entry of w is a zero array
    only = [t.numpy() for t in m32.pullback(None, torch.tensor(w[1]), None)]
    full = [t.numpy() for t in m32.pullback(torch.zeros_like(torch.tensor(w[0])), torch.tensor(w[1]), torch.zeros_like(torch.tensor(w[2])))]
    assert all(np.array_equal(a, b) for a, b in zip(only, full))


@pytest.mark.parametrize("cls_name", T.CLASSES)
def test_torch_diag_against_the_dense_jacobian(cls_name):
    v, w, h, m32, m64 = _pair(cls_name)
    J = T.jacobian64(m64)
    assert J.shape == (216, 45)
    got = [t.numpy() for t in m32.diag(*[torch.tensor(a) for a in h])]
    T.close(got, T.diag64(m64, h), T.tol_of(cls_name), cls_name + " torch diag against the dense Jacobian")


def test_diag_of_kind_0_on_an_interior_mask_is_the_cropped_pseudo_hessian_map():
    """Mask = 1 on the physical cells and 0 on the padding: no rim term, Mask^2 = 1 -- utils.pseudo_hessian_vp_vs_den, cropped."""
    from sepfwi import utils as ft
    nz, nx, nPml, nPad = T.SMALL
    v, w, h, m32, m64 = _pair("FWI", mask=T.interior_mask(T.SMALL))
    f = [getattr(m64, n).detach().numpy() for n in m64.NAMES]
    got = [t.numpy() for t in m32.diag(*[torch.tensor(a) for a in h])]
    pad = [torch.tensor(ft.padding_numpy_array(np.asarray(a, np.float32).astype(np.float64), nPml, nPad)) for a in f]
    ref = ft.pseudo_hessian_vp_vs_den(*[torch.tensor(a.astype(np.float64)) for a in h], *pad)
    ref = [t.numpy()[nPml:nPml + nz, nPml:nPml + nx] for t in ref]
    T.close(got, ref, T.tol_of("FWI"), "FWI torch diag against utils.pseudo_hessian_vp_vs_den, cropped")


# ---- PyTorchObjective.hessp on a stand-in: gauss_newton(v) = Q v for a fixed SPD Q, loss 1/2 (x - x*)^T Q (x - x*) ----------------
class _Quadratic(torch.nn.Module):
    NAMES = ("a", "b", "c")
    SHAPE = (2, 3)

    def __init__(self, Q, target, grads=(True, True, True)):
        super().__init__()
        self.Q, self.target, self.seen = Q, target, []
        for n, g in zip(self.NAMES, grads):
            t = torch.zeros(self.SHAPE, dtype=torch.float64)
            setattr(self, n, torch.nn.Parameter(t) if g else t)

    def flat(self):
        return torch.cat([getattr(self, n).reshape(-1) for n in self.NAMES])

    def loss(self):
        d = self.flat() - self.target
        return 0.5 * d @ (self.Q @ d)

    def gauss_newton(self, v, shot_ids, exact=False):
        self.seen.append((tuple(t is None for t in v), shot_ids, exact))
        x = torch.cat([torch.zeros(6, dtype=torch.float64) if t is None else t.reshape(-1) for t in v])
        return tuple((self.Q @ x).reshape(3, *self.SHAPE))


def _spd(rng, n=18):
    a = rng.standard_normal((n, n))
    return torch.tensor(a @ a.T + n * np.eye(n))


def test_hessp_is_q_p_and_trust_ncg_reaches_the_minimiser():
    from scipy import optimize
    from sepfwi.obj_wrapper import PyTorchObjective
    rng = np.random.default_rng(5)
    Q, target = _spd(rng), torch.tensor(rng.standard_normal(18))
    mod = _Quadratic(Q, target)
    obj = PyTorchObjective(mod, mod.loss, shot_ids="ids", exact=True)
    x, p = rng.standard_normal(18), rng.standard_normal(18)
    want = Q.numpy() @ p
    got = obj.hessp(x, p)
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert mod.seen[-1] == ((False, False, False), "ids", True)
    assert np.array_equal(mod.flat().detach().numpy(), x)          # x was loaded, as cache does
    res = optimize.minimize(obj.fun, obj.x0, jac=obj.jac, hessp=obj.hessp, method="trust-ncg", options={"gtol": 1e-10})
    assert np.abs(res.x - target.numpy()).max() <= 1e-8 * np.abs(target.numpy()).max(), res
    assert PyTorchObjective(mod, mod.loss, shot_ids="ids", exact=False).hessp(x, p) is not None and mod.seen[-1][2] is False


def test_hessp_packs_in_named_parameters_order_when_only_the_middle_field_is_inverted():
    from sepfwi.obj_wrapper import PyTorchObjective
    rng = np.random.default_rng(6)
    Q = _spd(rng)
    mod = _Quadratic(Q, torch.zeros(18, dtype=torch.float64), grads=(False, True, False))
    assert [n for n, _ in mod.named_parameters()] == ["b"]
    obj = PyTorchObjective(mod, mod.loss, shot_ids=[0])
    assert obj.x0.size == 6
    x, p = rng.standard_normal(6), rng.standard_normal(6)
    got = obj.hessp(x, p)
    want = Q.numpy()[6:12, 6:12] @ p
    assert got.shape == (6,) and np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert mod.seen[-1][0] == (True, False, True)                  # the fields that are no parameters get None


def test_hessp_refuses_without_shots_or_without_a_product():
    from sepfwi.obj_wrapper import PyTorchObjective
    Q = _spd(np.random.default_rng(7))
    mod = _Quadratic(Q, torch.zeros(18, dtype=torch.float64))
    two = PyTorchObjective(mod, mod.loss)                          # the two-argument form is unchanged
    assert two.shot_ids is None and two.fun(two.x0) == 0.0
    with pytest.raises(ValueError):
        two.hessp(two.x0, two.x0)
    plain = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError):
        PyTorchObjective(plain, lambda: plain.weight.sum(), shot_ids=[0]).hessp(np.zeros(6), np.zeros(6))
