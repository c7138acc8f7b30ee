"""The smoothing operator without a GPU: the torch path of sepfwi.smooth.Smoother (what CPU and float64 tensors run) against the dense
float64 definition (tests/smoother_ref.py), its identities, the two C-ABI entry points (exported, declared, every refusal before a device
is touched), gauss_newton_cg(precond=) on a small dense system and PyTorchObjective(smoother=) on a toy quadratic module.

Every test fails on the parent: sepfwi.smooth, the entry points and the two keyword arguments are missing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import smoother_ref as R
from conftest import ROOT

EINVAL = -1


def _ids(x):
    return "x".join(map(str, x)) if isinstance(x, tuple) else str(x)


def _t64(arrs):
    return tuple(None if a is None else torch.tensor(a, dtype=torch.float64) for a in arrs)


@pytest.mark.parametrize("kind", R.WIDTHS)
@pytest.mark.parametrize("grid", R.SMALL, ids=_ids)
def test_float64_torch_path_equals_the_dense_definition(grid, kind):
    """apply, apply_t and gram within 1e-13 of the largest reference entry; S 1 = 1 and <S u, y> = <u, S^T y> to 1e-13"""
    sm = R.smoother_of(grid, kind)
    ref = R.reference(grid, kind)
    sx, sz = R.widths(grid, kind)
    u = R.fields(grid)
    got_s, got_t, got_g = sm.apply(_t64(u)), sm.apply_t(_t64(u)), sm.gram(_t64(u))
    want_g = R.S(ref["St"], grid, sx, sz)
    for k in range(3):
        for what, got, want in (("S", got_s[k], ref["S"][k]), ("S^T", got_t[k], ref["St"][k]), ("S S^T", got_g[k], want_g[k])):
            dev = np.abs(got.numpy() - want).max() / np.abs(want).max()
            print("smoother %s %s field %d %s: %.2e of the largest entry" % (_ids(grid), kind, k, what, dev))
            assert got.dtype == torch.float64 and dev <= 1e-13
    one = sm.apply((torch.ones(grid[:2], dtype=torch.float64),))[0]
    assert float((one - 1.0).abs().max()) <= 1e-13
    y = R.fields(grid, seed=1)
    sy = sm.apply_t(_t64(y))
    for k in range(3):
        lhs, rhs = float((got_s[k] * torch.tensor(y[k], dtype=torch.float64)).sum()), float((torch.tensor(u[k], dtype=torch.float64) * sy[k]).sum())
        scale = float((torch.tensor(ref["Sabs"][k]) * torch.tensor(np.abs(y[k]), dtype=torch.float64)).sum())
        print("smoother %s %s field %d: <S u, y> %.12e, <u, S^T y> %.12e, difference %.2e of <S |u|, |y|>" % (_ids(grid), kind, k, lhs, rhs, abs(lhs - rhs) / scale))
        assert abs(lhs - rhs) <= 1e-13 * scale


def test_the_dense_definition_has_the_properties_of_the_header():
    """of the yardstick itself: S 1 = 1, the dot-product identity, S S^T symmetric and non-negative -- on explicit matrices"""
    grid, kind = (5, 65, 7, 32), "random"
    sx, sz = R.widths(grid, kind)
    n = grid[0] * grid[1]
    eye = [np.eye(n)[k].reshape(grid[:2]) for k in range(n)]
    M = np.stack([a.ravel() for a in R.S(eye, grid, sx, sz)], axis=1)             # S as a dense matrix, column by column
    Mt = np.stack([a.ravel() for a in R.St(eye, grid, sx, sz)], axis=1)
    assert np.abs(M.T - Mt).max() <= 1e-15 and np.abs(M.sum(axis=1) - 1.0).max() <= 1e-14 and M.min() >= 0.0
    G = M @ M.T
    assert np.abs(G - G.T).max() == 0.0 and np.linalg.eigvalsh(G).min() >= -1e-14


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_zero_width_gives_the_bits_of_the_input(dtype):
    from sepfwi.smooth import Smoother
    u = tuple(torch.tensor(a).to(dtype) for a in R.fields((5, 65)))
    for sm in (Smoother((5, 65), 0.0, 0.0, unit="cells"), Smoother((5, 65), 0.0, 0.0, unit="cells", radius=7), Smoother((5, 65), None, None, unit="cells")):
        for out in (sm.apply(u), sm.apply_t(u), sm.gram(u)):
            assert all(torch.equal(a, b) and a is not b for a, b in zip(out, u))
    # a zero patch among wide cells: S = I on the cells whose every tap pairs two zero widths (the sum of squares is not > 0), while
    # the patch's rim still trades with the wide cells next to it
    sig = torch.full((5, 65), 2.0)
    sig[:, 20:41] = 0.0
    sm = Smoother((5, 65), sig, None, unit="cells", radius=3)
    inner, rim = slice(23, 38), slice(20, 23)
    for a, b in zip(sm.apply(u) + sm.apply_t(u), u + u):
        assert torch.equal(a[:, inner], b[:, inner]) and not (a[:, rim] == b[:, rim]).any() and not (a[:, :20] == b[:, :20]).any()


def test_constant_width_is_a_truncated_gaussian_convolution():
    """sigma constant: K[j, m] = exp(-(m - j)^2 / (2 sigma^2)) for |m - j| <= r -- numpy.convolve with that stencil, normalised by the
    convolution of ones (the stencil's part inside the grid)"""
    from sepfwi.smooth import Smoother
    nz, nx, sigma, r = 6, 40, 2.5, 6
    sm = Smoother((nz, nx), sigma, None, unit="cells", radius=r)
    assert sm.radius == (6, 6) and Smoother((nz, nx), sigma, 1.0, unit="cells").radius == (8, 3)
    assert Smoother((nz, nx), 500.0, 30.0, dx=10.0, dz=20.0).radius == (64, 5)       # metres -> cells, min(64, ceil(3 sigma))
    stencil = np.exp(-np.arange(-r, r + 1) ** 2 / (2.0 * sigma ** 2))
    u = np.random.default_rng(2).standard_normal((nz, nx))
    want = np.stack([np.convolve(row, stencil, "same") / np.convolve(np.ones(nx), stencil, "same") for row in u])
    got = sm.apply((torch.tensor(u),))[0].numpy()
    assert np.abs(got - want).max() <= 1e-13


def test_call_is_differentiable_and_its_backward_is_the_transpose():
    grid, kind = (5, 65, 7, 32), "random"
    sm = R.smoother_of(grid, kind)
    u, y = (torch.tensor(a, dtype=torch.float64) for a in R.fields(grid)[:2])
    x = u.clone().requires_grad_(True)
    out = sm(x)
    assert out.requires_grad and torch.equal(out.detach(), sm.apply((u,))[0])
    (out * y).sum().backward()
    assert torch.equal(x.grad, sm.apply_t((y,))[0])
    # tuples pass None through; a bare tensor, a wrong shape and bad widths are refused
    full = sm.apply((u, None, y))
    assert full[1] is None and torch.equal(full[2], sm.apply((y,))[0])
    from sepfwi.smooth import Smoother
    with pytest.raises(ValueError):
        sm.apply(u)
    with pytest.raises(ValueError):
        sm.apply((torch.zeros(2, 2),))
    for bad in (dict(sigma_x=-1.0), dict(sigma_x=float("nan")), dict(sigma_z=float("inf")), dict(sigma_x=torch.zeros(3, 3)), dict(radius=65),
                dict(radius=(-1, 2)), dict(unit="feet")):
        with pytest.raises(ValueError):
            Smoother(**{"module_or_shape": (5, 65), "sigma_x": 1.0, "sigma_z": 1.0, "unit": "cells", **bad})
    with pytest.raises(ValueError):
        Smoother((5, 65), 10.0, 10.0)           # metres without dx, dz


def test_module_constructor_and_from_wavelength(tmp_path):
    import problems as P
    from sepfwi import modules as M
    from sepfwi.smooth import Smoother
    pb = P.make_problem(str(tmp_path), nz=12, nx=16, nPml=4, nSteps=10, nshots=1, dh=10.0, dz=8.0)
    f = [torch.tensor(pb["init"][k], requires_grad=True) for k in ("vp", "vs", "rho")]
    fwi = M.FWI(f[0], f[1], f[2], pb["Stf"], pb["opt"])
    sm = Smoother(fwi, 20.0, 16.0)
    assert (sm.dx, sm.dz) == (10.0, 8.0) and sm.shape == (12, 16) and sm.names == tuple(fwi.NAMES) and sm.radius == (6, 6)
    assert float(sm.sigma[0].max()) == 2.0 and float(sm.sigma[1].min()) == 2.0
    vs = torch.tensor(pb["init"]["vs"])
    wl = Smoother.from_wavelength(fwi, vs, fmax=25.0, fraction=0.5)
    assert torch.equal(wl.sigma[0], (vs.double() * (0.5 / 25.0) / 10.0).float()) and torch.equal(wl.sigma[1], (vs.double() * (0.5 / 25.0) / 8.0).float())
    out = wl.apply(tuple(getattr(fwi, n).detach() for n in fwi.NAMES))
    assert len(out) == 3 and all(torch.isfinite(t).all() for t in out)


def test_preconditioner_is_symmetric_and_floors_the_diagonal():
    grid, kind = (5, 65, 7, 32), "random"
    sm = R.smoother_of(grid, kind)
    a, b = _t64(R.fields(grid)), _t64(R.fields(grid, seed=1))
    D = [torch.rand(grid[:2], dtype=torch.float64, generator=torch.Generator().manual_seed(k)) for k in range(3)]
    D[1][:2] = 0.0
    D[2][0, :5] = -1.0
    prec = sm.preconditioner(D)
    dot = lambda x, y: float(sum((p * q).sum() for p, q in zip(x, y)))
    pa, pb_ = prec(a), prec(b)
    assert isinstance(pa, list) and abs(dot(b, pa) - dot(a, pb_)) <= 1e-12 * abs(dot(b, pa)) and dot(a, pa) > 0
    floor = lambda d: d.clamp_min(0).clamp_min(1e-12 * float(d.clamp_min(0).max()))
    want = [g / floor(d).sqrt() for g, d in zip(sm.gram(tuple(x / floor(d).sqrt() for x, d in zip(a, D))), D)]
    assert all(float((x - y).abs().max()) <= 1e-12 * float(y.abs().max()) for x, y in zip(pa, want))
    plain = sm.preconditioner()(a)
    assert all(torch.equal(x, y) for x, y in zip(plain, sm.gram(a)))


def test_symbols_are_exported_declared_and_refuse_without_a_device(tmp_path):
    from sepfwi import _native
    L = _native.lib()
    for name, nargs in (("sepfwi_smooth_plan", 9), ("sepfwi_smooth_apply", 12)):
        assert name in _native.EXPORTS
        f = getattr(L, name)
        assert f.restype is C.c_int and len(f.argtypes) == nargs
    inc = os.path.join(ROOT, "include")
    body = ('#include "sepfwi.h"\nint call(const float *s, float *w, const float *const p[3], float *const q[3]) {\n'
            '    return sepfwi_smooth_plan(1, 1, 0, 0, s, s, w, w, 0) + sepfwi_smooth_apply(1, 1, 0, 0, s, s, w, w, 1, p, q, 0);\n}\n')
    (tmp_path / "t.c").write_text(body)
    (tmp_path / "t.cpp").write_text(body)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", inc, str(tmp_path / "t.c")])
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", inc, str(tmp_path / "t.cpp")])

    grid = (2, 3, 1, 1)
    sx, sz = R.widths(grid, "constant")
    u = R.fields(grid)
    inv = np.ones((2, 3), np.float32)
    refused = lambda rc: rc == EINVAL and b"smoother" in L.sepfwi_last_error()

    def plan(g=grid, sigx=sx, sigz=sz, inv=("auto", "auto")):
        return refused(R.c_plan(L, g, sigx, sigz, inv=inv)[0])

    def apply(g=grid, p=(sx, sz, inv, inv), fields=u, outs="auto", transpose=0):
        src = [None if a is None else a.copy() for a in fields]
        dst = [None if a is None else np.empty_like(a) for a in fields] if outs == "auto" else outs
        return refused(L.sepfwi_smooth_apply(g[0], g[1], g[3], g[2], *[R._ptr(a) for a in p], transpose, R._triple(src), R._triple(dst), None))

    for call in (plan, apply):
        assert call(g=(0, 3, 1, 1)) and call(g=(2, 0, 1, 1)) and call(g=(-2, 3, 1, 1))            # nz, nx < 1
        assert call(g=(2, 3, -1, 1)) and call(g=(2, 3, 1, -1)) and call(g=(2, 3, 65, 1)) and call(g=(2, 3, 1, 65))      # a radius outside 0 .. 64
    assert plan(inv=(None, "auto")) and plan(inv=("auto", None))                                    # widths without their inv_*
    assert apply(p=(sx, sz, None, inv)) and apply(p=(sx, sz, inv, None))
    for t in (0, 1):
        assert apply(fields=[None, None, None], transpose=t)                                        # all three fields NULL
        assert apply(outs=[np.empty_like(u[0]), None, np.empty_like(u[2])], transpose=t)            # in[1] without out[1]
        assert apply(fields=[u[0], None, None], outs=[np.empty_like(u[0]), np.empty_like(u[0]), None], transpose=t)     # out[1] without in[1]
    assert refused(L.sepfwi_smooth_apply(2, 3, 1, 1, R._ptr(sx), R._ptr(sz), R._ptr(inv), R._ptr(inv), 0, None, None, None))   # NULL triples
    # a plan without any width array has nothing to do and touches nothing
    assert L.sepfwi_smooth_plan(2, 3, 1, 1, None, None, None, None, None) == 0


def _spd(n, seed):
    """a dense SPD system whose ill-conditioning lives in the rough directions of a 1-D grid: A = (I + c L)^2, L the second-difference
    matrix -- what a smoothing preconditioner is for"""
    L = 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)
    B = np.eye(n) + 30.0 * L
    rng = np.random.default_rng(seed)
    return torch.tensor(B @ B), torch.tensor(rng.standard_normal(n))


def test_gauss_newton_cg_takes_a_preconditioner():
    from sepfwi.obj_wrapper import gauss_newton_cg
    from sepfwi.smooth import Smoother
    n = 96
    A, g = _spd(n, 5)
    hessvec = lambda v: [(A @ v[0].reshape(-1)).reshape(1, n)]
    grad = [g.reshape(1, n)]
    sm = Smoother((1, n), 1.0, None, unit="cells")
    want = -torch.linalg.solve(A, g)
    err = lambda p: float((p[0].reshape(-1) - want).norm() / want.norm())
    p0, h0 = gauss_newton_cg(hessvec, grad, maxiter=400, rtol=1e-10)
    p1, h1 = gauss_newton_cg(hessvec, grad, maxiter=400, rtol=1e-10, precond=sm.preconditioner())
    print("cg on (I + 30 L)^2, n = %d: %d iterations without, %d with S S^T; errors %.2e, %.2e" % (n, len(h0) - 1, len(h1) - 1, err(p0), err(p1)))
    assert err(p1) <= 1e-7 and h1[-1] <= 1e-10 and len(h1) < len(h0)
    # diag keeps its role in the damping term while precond replaces the Jacobi preconditioner
    D = [torch.linspace(0.5, 2.0, n, dtype=torch.float64).reshape(1, n)]
    p2, _ = gauss_newton_cg(hessvec, grad, damping=0.3, diag=D, maxiter=400, rtol=1e-12, precond=sm.preconditioner(D))
    want2 = -torch.linalg.solve(A + 0.3 * torch.diag(D[0].reshape(-1)), g)
    assert float((p2[0].reshape(-1) - want2).norm() / want2.norm()) <= 1e-7
    # precond=None: the bits of the call without the argument, with and without a diagonal
    for kw in (dict(), dict(diag=D, damping=0.3)):
        a, ha = gauss_newton_cg(hessvec, grad, maxiter=25, rtol=1e-30, **kw)
        b, hb = gauss_newton_cg(hessvec, grad, maxiter=25, rtol=1e-30, precond=None, **kw)
        assert torch.equal(a[0], b[0]) and ha == hb and len(ha) == 26


class Quadratic(torch.nn.Module):
    """three (nz, nx) fields A, B, C (C is no parameter) with loss sum_k c_k |W (p_k - t_k)|^2 / 2 + a coupling of A and B: its
    Gauss-Newton product is its Hessian"""
    NAMES = ("A", "B", "C")
    para_fname = None

    def __init__(self, shape, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        rnd = lambda: torch.randn(shape, dtype=torch.float64, generator=g)
        self.A = torch.nn.Parameter(3000.0 + 50.0 * rnd())
        self.B = torch.nn.Parameter(1700.0 + 30.0 * rnd())
        self.C = torch.full(shape, 2400.0, dtype=torch.float64)
        self.tA, self.tB, self.W = 3000.0 + 50.0 * rnd(), 1700.0 + 30.0 * rnd(), 0.5 + torch.rand(shape, dtype=torch.float64, generator=g)

    def loss(self):
        dA, dB = self.W * (self.A - self.tA), self.W * (self.B - self.tB)
        return 0.5 * (1e-3 * (dA * dA).sum() + 2e-3 * (dB * dB).sum() + 1e-3 * (dA * dB).sum())

    def gauss_newton(self, v, ids, exact=True):
        w2 = self.W * self.W
        return (1e-3 * w2 * v[0] + 0.5e-3 * w2 * v[1], 2e-3 * w2 * v[1] + 0.5e-3 * w2 * v[0], None)


def test_objective_in_the_smoothed_variables():
    """PyTorchObjective(smoother=): x0 = 0 loads p_ref; central differences of fun in y meet jac to 1e-6 of |jac| along random
    directions (the loss is quadratic: the differences are exact up to rounding); hessp is symmetric and is the Hessian in y."""
    from sepfwi.obj_wrapper import PyTorchObjective
    grid, kind = (5, 65, 7, 32), "random"
    sm = R.smoother_of(grid, kind)
    mod = Quadratic(grid[:2])
    ref = [mod.A.detach().clone(), mod.B.detach().clone()]
    obj = PyTorchObjective(mod, mod.loss, shot_ids=[0], smoother=sm)
    plain = PyTorchObjective(Quadratic(grid[:2]), mod.loss, shot_ids=[0])
    n = 2 * 5 * 65
    assert obj.bounds is None and obj.x0.shape == (n,) and not obj.x0.any() and plain.x0.any() and "separable" in PyTorchObjective.__doc__
    assert list(obj.scales) == ["A", "B"] and obj.scales["A"] == float(ref[0].abs().mean()) and obj.scales["B"] == float(ref[1].abs().mean())
    fun, jac = obj.fun, obj.jac              # (the first evaluation caches the gradient under the method's name, as the reference does)
    f0 = fun(obj.x0)
    assert torch.equal(mod.A.detach(), ref[0]) and torch.equal(mod.B.detach(), ref[1]) and f0 == float(mod.loss().detach())
    rng = np.random.default_rng(4)
    y = 1e-3 * rng.standard_normal(n)
    g = np.array(jac(y))
    # the loaded model is p_ref + s S y
    Sy = sm.apply((torch.tensor(y[:325].reshape(5, 65)), torch.tensor(y[325:].reshape(5, 65))))
    assert torch.equal(mod.A.detach(), ref[0] + obj.scales["A"] * Sy[0]) and torch.equal(mod.B.detach(), ref[1] + obj.scales["B"] * Sy[1])
    for k in range(3):
        d = rng.standard_normal(n)
        h = 1e-4
        fd = (fun(y + h * d) - fun(y - h * d)) / (2 * h)
        print("objective in y: direction %d, central difference %.10e, <jac, d> %.10e, off by %.2e of |jac| |d|" % (
            k, fd, g @ d, abs(fd - g @ d) / (np.linalg.norm(g) * np.linalg.norm(d))))
        assert abs(fd - g @ d) <= 1e-6 * np.linalg.norm(g) * np.linalg.norm(d)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    ha, hb = obj.hessp(y, a), obj.hessp(y, b)
    assert ha.dtype == np.float64 and ha.shape == (n,)
    print("objective in y: <b, H a> %.12e, <a, H b> %.12e" % (b @ ha, a @ hb))
    assert abs(b @ ha - a @ hb) <= 1e-12 * abs(b @ ha) and a @ ha > 0
    # quadratic loss: jac(y + a) - jac(y) = H a
    dg = np.array(jac(y + a)) - g
    assert np.abs(dg - ha).max() <= 1e-9 * np.abs(ha).max()
    # scales= as a number, a tuple, a dict; bad ones refused
    assert list(PyTorchObjective(mod, mod.loss, smoother=sm, scales=2.0).scales.values()) == [2.0, 2.0]
    assert list(PyTorchObjective(mod, mod.loss, smoother=sm, scales=(2.0, 3.0)).scales.values()) == [2.0, 3.0]
    assert list(PyTorchObjective(mod, mod.loss, smoother=sm, scales={"B": 5.0, "A": 4.0}).scales.values()) == [4.0, 5.0]
    for bad in (0.0, (1.0,), (1.0, -2.0)):
        with pytest.raises(ValueError):
            PyTorchObjective(mod, mod.loss, smoother=sm, scales=bad)


def test_objective_with_a_smoother_carries_the_regularizer_product():
    """hessp = s S^T (H + H_R) (s S p): the regulariser's product sits inside the change of variables"""
    from sepfwi.obj_wrapper import PyTorchObjective
    from sepfwi.regularize import Regularizer
    grid, kind = (5, 65, 7, 32), "constant"
    sm = R.smoother_of(grid, kind)
    mod = Quadratic(grid[:2], seed=3)
    reg = Regularizer(mod, beta=0.7, dx=10.0, dz=10.0)
    loss = lambda: mod.loss() + reg()
    with_reg = PyTorchObjective(mod, loss, shot_ids=[0], regularizer=reg, smoother=sm)
    without = PyTorchObjective(mod, loss, shot_ids=[0], smoother=sm)
    rng = np.random.default_rng(9)
    p = rng.standard_normal(with_reg.x0.size)
    v = with_reg.smoothed(with_reg.unpack_parameters(p))
    hr = reg.hvp((v["A"], v["B"], None))
    back = with_reg.smoothed({"A": hr[0], "B": hr[1]}, transpose=True)
    want = without.hessp(with_reg.x0, p) + np.concatenate([back["A"].numpy().ravel(), back["B"].numpy().ravel()])
    got = with_reg.hessp(with_reg.x0, p)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max() and np.abs(got - without.hessp(with_reg.x0, p)).max() > 0
