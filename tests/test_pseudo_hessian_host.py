"""Host side of the diagonal pseudo-Hessian (CPU only; no kernel is launched): the two C-ABI entry points without a device, the map of
the (Lambda, Mu, Den) result to (Vp, Vs, Den), and the variable scaling of obj_wrapper.minimize_lbfgsb."""
import numpy as np
import pytest
import torch
from scipy import optimize

import problems as P


def test_c_abi_entry_points_without_a_device(tmp_path):
    """Both symbols are exported; every < 0 is SEPFWI_EINVAL before anything is touched; asking for a result (or disarming) without a
    session needs no device."""
    from sepfwi import _native
    L = _native.lib()
    assert hasattr(L, "sepfwi_pseudo_hessian_arm") and hasattr(L, "sepfwi_get_pseudo_hessian")
    pb = P.make_problem(str(tmp_path), nSteps=20)
    fn = pb["para_fname"].encode()
    assert L.sepfwi_pseudo_hessian_arm(fn, 0, -1) == -1 and b"every" in L.sepfwi_last_error()       # SEPFWI_EINVAL
    assert L.sepfwi_pseudo_hessian_arm(b"/nonexistent/para.json", 0, -1) == -1 and b"every" in L.sepfwi_last_error()   # ... before the file is read
    out = np.zeros((pb["nz_pad"], pb["nx_pad"]), np.float32)
    assert L.sepfwi_get_pseudo_hessian(fn, 0, out.ctypes.data, None, None) == -1 and b"no session" in L.sepfwi_last_error()
    assert L.sepfwi_pseudo_hessian_arm(fn, 0, 0) == 0                                                # nothing to disarm: no session is made
    assert L.sepfwi_get_pseudo_hessian(fn, 0, None, None, None) == -1 and b"no session" in L.sepfwi_last_error()
    assert L.sepfwi_get_pseudo_hessian(None, 0, None, None, None) == -1


def test_operator_refuses_a_negative_stride_before_the_library_is_called(tmp_path):
    from sepfwi import fwi_ops
    pb = P.make_problem(str(tmp_path), nSteps=20)
    with pytest.raises(ValueError, match="pseudo_hessian"):
        fwi_ops.backward(*pb["lame_init"], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], pseudo_hessian=-1)


def test_vp_vs_den_map_is_the_weighted_column_sum_of_squares_of_the_jacobian():
    from sepfwi import utils as ft
    g = torch.Generator().manual_seed(3)
    shape = (5, 7)
    vp = 2500.0 + 1500.0 * torch.rand(shape, generator=g, dtype=torch.float64)
    vs = vp / (1.6 + 0.3 * torch.rand(shape, generator=g, dtype=torch.float64))
    den = 2000.0 + 700.0 * torch.rand(shape, generator=g, dtype=torch.float64)
    H = torch.rand((3,) + shape, generator=g, dtype=torch.float64) * torch.tensor([1e-3, 1.0, 1e3], dtype=torch.float64)[:, None, None]

    def lame(m):    # FWI_ops.py:124-125
        return torch.stack([(m[0] ** 2 - 2.0 * m[1] ** 2) * m[2] / 1e6, m[1] ** 2 * m[2] / 1e6, m[2]])

    J = torch.autograd.functional.jacobian(lame, torch.stack([vp, vs, den]))        # [out, z, x, in, z', x']
    want = torch.einsum("iab,iabjzx->jzx", H, J ** 2)
    got = ft.pseudo_hessian_vp_vs_den(H[0], H[1], H[2], vp, vs, den)
    for k in range(3):
        assert (want[k] > 0).all()
        np.testing.assert_allclose(got[k].numpy(), want[k].numpy(), rtol=1e-12, atol=0.0)


def _quadratic(n=40, cond=1e8, seed=5):
    """f = 0.5 sum d_i (x_i - c_i)^2 with d from 1 to cond, box [-1, 1]^n, a quarter of the minimisers outside the box."""
    rng = np.random.default_rng(seed)
    d = np.logspace(0.0, np.log10(cond), n)
    rng.shuffle(d)
    c = rng.uniform(-0.9, 0.9, n)
    c[::4] = rng.choice([-1.5, 1.5], c[::4].size)
    fun = lambda x: 0.5 * float((d * (x - c) ** 2).sum())
    jac = lambda x: d * (x - c)
    return d, c, fun, jac, optimize.Bounds(-np.ones(n), np.ones(n))


def test_unit_scale_gives_the_iterates_of_no_scale():
    from sepfwi.obj_wrapper import minimize_lbfgsb
    d, c, fun, jac, bounds = _quadratic(cond=1e3)
    runs = []
    for scale in (None, np.ones(d.size)):
        its = []
        res = minimize_lbfgsb(fun, np.zeros(d.size), jac, bounds=bounds, callback=lambda x: its.append(x.copy()), maxiter=30, scale=scale)
        runs.append((its, res))
    (a, ra), (b, rb) = runs
    assert len(a) == len(b) >= 3 and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(ra.x, rb.x) and ra.fun == rb.fun and ra.nit == rb.nit


def test_scaling_by_the_diagonal_conditions_a_bounded_quadratic():
    """Condition number 1e8, scale = diag^(-1/2): in y = x / scale the quadratic is perfectly conditioned, the scaled run meets gtol in
    fewer iterations than the unscaled one; the result is in x and inside the ORIGINAL box."""
    from sepfwi.obj_wrapper import minimize_lbfgsb
    d, c, fun, jac, bounds = _quadratic()
    kw = dict(bounds=bounds, maxiter=1000, maxfun=20000, ftol=0.0, gtol=1e-6)
    plain = minimize_lbfgsb(fun, np.zeros(d.size), jac, **kw)
    seen = []
    scaled = minimize_lbfgsb(fun, np.zeros(d.size), jac, scale=d ** -0.5, callback=lambda x: seen.append(x.copy()), **kw)
    print("bounded quadratic, cond 1e8: %d iterations unscaled (%s), %d scaled (%s)" % (plain.nit, plain.message, scaled.nit, scaled.message))
    assert scaled.success and "PROJECTED GRADIENT" in scaled.message
    assert scaled.nit < plain.nit
    assert (scaled.x >= bounds.lb).all() and (scaled.x <= bounds.ub).all()
    assert all(((x >= bounds.lb) & (x <= bounds.ub)).all() for x in seen) and np.array_equal(seen[-1], scaled.x)    # the callback sees x
    want = np.clip(c, -1.0, 1.0)
    assert np.abs(scaled.x - want).max() <= 1e-6
    assert scaled.fun <= plain.fun + 1e-9


def test_scale_must_be_positive_and_of_the_right_size():
    from sepfwi.obj_wrapper import minimize_lbfgsb
    d, c, fun, jac, bounds = _quadratic(n=8)
    for bad in (np.ones(7), -np.ones(8), np.zeros(8)):
        with pytest.raises(ValueError):
            minimize_lbfgsb(fun, np.zeros(8), jac, bounds=bounds, scale=bad)
