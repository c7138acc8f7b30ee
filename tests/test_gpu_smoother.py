"""The smoothing operator on the GPU (-m gpu): k_smooth_norm, k_smooth_x and k_smooth_z of csrc/smoother.hip through sepfwi_smooth_plan /
sepfwi_smooth_apply, sepfwi.smooth.Smoother on HIP tensors, and one run of each example flag.

Reference: the dense float64 definition (tests/smoother_ref.py), inputs born float32.  Bounds, with T = (2 rx + 1) + (2 rz + 1) and
u = 2^-24:
  S      max |got - ref| <= (T + 16) u max |in|: the running-error bound of two normalised sums of non-negative terms plus the roundings of
         the exponential's argument, the reciprocal and the scaling;
  S^T    the same with max (S^T |in|) of the reference in place of max |in|;
  dot    |<S a, b> - <a, S^T b>| <= (T + 16) u <S |a|, |b|>, the dots in float64;
  S 1    within 4 u of 1;
  gram   |<a, S S^T b> - <b, S S^T a>| <= 2 (T + 16) u <|a|, S S^T |b|>: each side carries two applications.
Bit identities need no bound.  Every comparison prints its figure before it asserts (profiles/r26_smoother.txt holds those measured on the
MI355X).  Sequential float32 numpy sits at 0.008 - 0.035 of the S bound and a dropped outermost tap at 190 - 7400 times it, so a figure
above a bound is a defect, not a tolerance to widen.

Every test fails on the parent: the entry points and sepfwi.smooth are missing."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import smoother_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

U = R.U
# every width kind on the small grids; the several-tile grid with the two kinds that exercise every tap
CASES = [(g, k) for g in R.SMALL for k in R.WIDTHS] + [(R.GRIDS[5], "random"), (R.GRIDS[5], "zero_patch")]


def _ids(x):
    return "x".join(map(str, x)) if isinstance(x, tuple) else str(x)


def _lib(hip_ops):
    from sepfwi import _native
    return _native.lib()


def _dot(a, b):
    return float((np.asarray(a, np.float64) * np.asarray(b, np.float64)).sum())


def _same(a, b):
    return all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y)) for x, y in zip(a, b))


@pytest.mark.parametrize("grid,kind", CASES, ids=["%s-%s" % (_ids(g), k) for g, k in CASES])
def test_kernels_against_the_float64_definition(hip_ops, grid, kind):
    L = _lib(hip_ops)
    bound = (R.taps(grid) + 16) * U
    sx, sz = R.widths(grid, kind)
    a, b = R.fields(grid), R.fields(grid, seed=1)
    ref, ref_b = R.reference(grid, kind), R.reference(grid, kind, seed=1)
    rc, plan = R.c_plan(L, grid, sx, sz, on_device=True)
    assert rc == 0, L.sepfwi_last_error()
    rc, s_a = R.c_apply(L, grid, plan, a, False, on_device=True)
    assert rc == 0, L.sepfwi_last_error()
    rc, t_b = R.c_apply(L, grid, plan, b, True, on_device=True)
    assert rc == 0, L.sepfwi_last_error()
    for k in range(3):
        dev, top = np.abs(s_a[k] - ref["S"][k]).max(), float(np.abs(a[k]).max())
        print("smoother %s %s field %d: S off by %.3e = %.4f of the bound %.3e" % (_ids(grid), kind, k, dev, dev / (bound * top), bound * top))
        assert s_a[k].dtype == np.float32 and dev <= bound * top
        dev, top = np.abs(t_b[k] - ref_b["St"][k]).max(), float(ref_b["Stabs"][k].max())
        print("smoother %s %s field %d: S^T off by %.3e = %.4f of the bound %.3e" % (_ids(grid), kind, k, dev, dev / (bound * top), bound * top))
        assert dev <= bound * top
        lhs, rhs, scale = _dot(s_a[k], b[k]), _dot(a[k], t_b[k]), _dot(ref["Sabs"][k], np.abs(b[k]))
        print("smoother %s %s field %d: <S a, b> %.10e, <a, S^T b> %.10e, difference %.3e = %.4f of the bound %.3e" % (
            _ids(grid), kind, k, lhs, rhs, abs(lhs - rhs), abs(lhs - rhs) / (bound * scale), bound * scale))
        assert abs(lhs - rhs) <= bound * scale
    one = np.ones(grid[:2], np.float32)
    rc, s_one = R.c_apply(L, grid, plan, [one, None, None], False, on_device=True)
    dev = np.abs(s_one[0].astype(np.float64) - 1.0).max()
    print("smoother %s %s: S 1 off by %.3e = %.2f u (bound 4 u)" % (_ids(grid), kind, dev, dev / U))
    assert rc == 0 and dev <= 4 * U

    # bit identities: host pointers, a second call, one field at a time with NULL gaps, in place
    rc, hplan = R.c_plan(L, grid, sx, sz, on_device=False)
    assert rc == 0 and _same([R.host(x) for x in hplan[2:]], [R.host(x) for x in plan[2:]])
    for transpose, src, want in ((False, a, s_a), (True, b, t_b)):
        rc, h = R.c_apply(L, grid, hplan, src, transpose, on_device=False)
        assert rc == 0 and _same(h, want), "host pointers"
        rc, again = R.c_apply(L, grid, plan, src, transpose, on_device=True)
        assert rc == 0 and _same(again, want), "a second call"
        for present in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)):
            part = [x if on else None for x, on in zip(src, present)]
            rc, got = R.c_apply(L, grid, plan, part, transpose, on_device=True)
            assert rc == 0 and _same(got, [x if on else None for x, on in zip(want, present)]), present
        rc, inp = R.c_apply(L, grid, plan, src, transpose, on_device=True, in_place=True)
        assert rc == 0 and _same(inp, want), "in place"
        rc, inp = R.c_apply(L, grid, hplan, src, transpose, on_device=False, in_place=True)
        assert rc == 0 and _same(inp, want), "in place, host pointers"


def test_identity_axes_and_mixed_pointers(hip_ops):
    """radius 0 or no widths: that axis is the identity, both: the input's bits (in place too); single arrays may live on the host"""
    L = _lib(hip_ops)
    grid = (5, 65, 7, 32)
    sx, sz = R.widths(grid, "random")
    a = R.fields(grid)
    rc, plan = R.c_plan(L, grid, sx, sz, on_device=True)
    rc, want = R.c_apply(L, grid, plan, a, False, on_device=True)
    for g0, p0 in (((5, 65, 0, 0), plan), (grid, (None, None, None, None)), ((5, 65, 0, 32), (None, plan[1], None, plan[3]))):
        for in_place in (False, True):
            for transpose in (False, True):
                rc, got = R.c_apply(L, g0, p0, a, transpose, on_device=True, in_place=in_place)
                assert rc == 0 and _same(got, a), (g0, in_place, transpose)
    # z only == the x radius 0; x only == no z widths
    rc, z_only = R.c_apply(L, (5, 65, 7, 0), plan, a, False, on_device=True)
    rc2, z_null = R.c_apply(L, grid, (None, plan[1], None, plan[3]), a, False, on_device=True)
    rc3, z_inp = R.c_apply(L, (5, 65, 7, 0), plan, a, False, on_device=True, in_place=True)
    ref_z = R.S(a, grid, None, sz)
    assert rc == 0 and rc2 == 0 and rc3 == 0 and _same(z_only, z_null) and _same(z_only, z_inp)
    assert all(np.abs(x - y).max() <= (R.taps(grid) + 16) * U * np.abs(u).max() for x, y, u in zip(z_only, ref_z, a))
    # the widths from the host, one input from the host, one output to the host
    import ctypes as C
    src = [torch.tensor(a[0]).cuda(), a[1].copy(), torch.tensor(a[2]).cuda()]
    dst = [np.empty_like(a[0]), torch.empty(a[1].shape, device="cuda"), torch.empty(a[2].shape, device="cuda")]
    rc = L.sepfwi_smooth_apply(5, 65, 32, 7, R._ptr(sx), R._ptr(plan[1]), R._ptr(plan[2]), R._ptr(R.host(plan[3]).copy()), 0, R._triple(src), R._triple(dst), None)
    torch.cuda.synchronize()
    assert rc == 0, L.sepfwi_last_error()
    assert _same([R.host(x) for x in dst], want)
    # release_all frees the intermediates; the next call allocates again
    dev0 = C.c_longlong(0)
    pin = C.c_longlong(0)
    L.sepfwi_release_all()
    L.sepfwi_debug_live_bytes(C.byref(dev0), C.byref(pin))
    rc, again = R.c_apply(L, grid, plan, a, False, on_device=True)
    dev1 = C.c_longlong(0)
    L.sepfwi_debug_live_bytes(C.byref(dev1), C.byref(pin))
    assert rc == 0 and _same(again, want) and dev1.value - dev0.value == 3 * 5 * 65 * 4
    L.sepfwi_release_all()
    L.sepfwi_debug_live_bytes(C.byref(dev1), C.byref(pin))
    assert dev1.value == dev0.value


@pytest.mark.parametrize("grid,kind", [((5, 65, 7, 32), "random"), ((67, 9, 32, 3), "z_null"), (R.GRIDS[5], "random")], ids=["5x65", "67x9-z_null", "300x500"])
def test_smoother_on_hip_tensors(hip_ops, grid, kind):
    """apply, apply_t and gram are the C calls bit for bit; the backward of __call__ is apply_t; gram is symmetric"""
    L = _lib(hip_ops)
    sm = R.smoother_of(grid, kind)
    sx, sz = R.widths(grid, kind)
    a, b = R.fields(grid), R.fields(grid, seed=1)
    cu = lambda arrs: tuple(None if x is None else torch.tensor(x).cuda() for x in arrs)
    rc, plan = R.c_plan(L, grid, sx, sz, on_device=True)
    rc, s_a = R.c_apply(L, grid, plan, a, False, on_device=True)
    rc2, t_a = R.c_apply(L, grid, plan, a, True, on_device=True)
    rc3, g_a = R.c_apply(L, grid, plan, t_a, False, on_device=True)
    assert rc == 0 and rc2 == 0 and rc3 == 0
    out_s, out_t, out_g = sm.apply(cu(a)), sm.apply_t(cu(a)), sm.gram(cu(a))
    assert all(t.is_cuda and t.dtype == torch.float32 for t in out_s + out_t + out_g)
    assert _same([R.host(t) for t in out_s], s_a) and _same([R.host(t) for t in out_t], t_a) and _same([R.host(t) for t in out_g], g_a)
    gap = sm.apply((cu(a)[0], None, cu(a)[2]))
    assert gap[1] is None and _same([R.host(gap[0]), R.host(gap[2])], [s_a[0], s_a[2]])
    x = cu(a)[0].clone().requires_grad_(True)
    y = cu(b)[0]
    (sm(x) * y).sum().backward()
    assert torch.equal(x.grad, sm.apply_t((y,))[0])
    g_b = sm.gram(cu(b))
    g_abs = R.S(R.reference(grid, kind, seed=1)["Stabs"], grid, sx, sz)
    bound = 2 * (R.taps(grid) + 16) * U
    for k in range(3):
        lhs, rhs, scale = _dot(a[k], R.host(g_b[k])), _dot(b[k], g_a[k]), _dot(np.abs(a[k]), g_abs[k])
        print("smoother %s %s field %d: <a, S S^T b> %.10e, <b, S S^T a> %.10e, difference %.3e = %.4f of the bound %.3e" % (
            _ids(grid), kind, k, lhs, rhs, abs(lhs - rhs), abs(lhs - rhs) / (bound * scale), bound * scale))
        assert abs(lhs - rhs) <= bound * scale and _dot(a[k], g_a[k]) > 0


def _run(script, extra, tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", script), "--device", "cuda", "--workdir", str(tmp_path)] + extra,
                         capture_output=True, text=True, timeout=500, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    its = [ln for ln in out.stdout.splitlines() if ln.startswith("iterate ")]
    return [float(ln.split("misfit")[1].split()[0]) for ln in its], out.stdout


def test_gauss_newton_example_with_the_smoothing_preconditioner(tmp_path):
    """examples/gauss_newton_fwi.py --smooth-precond 0.5 at the settings of tests/test_gpu_born_example.py: the misfit falls"""
    f, text = _run("gauss_newton_fwi.py", ["--outer", "2", "--inner", "3", "--nsteps", "700", "--shot-stride", "3", "--rtol", "1e-6", "--exact-adjoint",
                                           "--smooth-precond", "0.5"], tmp_path)
    assert "smoothing preconditioner: sigma" in text and len(f) >= 2 and np.isfinite(f).all() and f[-1] < f[0]
    res = [float(ln.split("relative residual")[1]) for ln in text.splitlines() if "relative residual" in ln]
    assert len(res) >= 3 and np.isfinite(res).all()


def test_anomaly_example_in_the_smoothed_variables(tmp_path):
    """examples/fwi_anomaly_vp_vs_den.py --smooth 60 at the settings of tests/test_gpu_pseudo_hessian.py's example run: the misfit falls"""
    f, text = _run("fwi_anomaly_vp_vs_den.py", ["--niter", "3", "--smooth", "60"], tmp_path)
    assert len(f) >= 2 and np.isfinite(f).all() and f[-1] < f[0]
    peak = float(text.split("recovered Vp anomaly peak")[1].split()[0])
    assert np.isfinite(peak)
