"""The inputs of tests/test_gpu_exact_adjoint.py kept honest without a GPU (CPU oracle only).

  * the pairs of perturbations whose cross products the GPU tests compare are neither parallel nor orthogonal in data space:
    |cos(J v1, J v2)| >= 0.1 per component that carries a weight (measured on PROBLEM_A: ett -0.32, vx -0.36);
  * the test can fail: the reference's own adjoint (the oracle's gradient at obs = syn - J v) misses v^T H v = |W^1/2 J v|^2 on the same
    inputs by at least 5 x the tolerance the exact adjoint is held to (7.7e-3 on PROBLEM_A for the unmasked v, profiles/r09_born.txt);
  * the single-cell probes of the cell-by-cell test are cells the wave reaches within the record: |J e_k| > 1e-6 of the largest
    (a cell in the far corner reads about 1e-28 within 260 steps);
  * the new symbol is exported, the header still compiles as C99 and C++17, and the device-free refusals are reached without a device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import exact_adjoint_ref as X
import problems as P
import pseudo_hessian_ref as R
from born_ref import GRADS, born_side, shifted_gradient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def prob_a(oracle, tmp_path_factory):
    pb = P.make_problem(str(tmp_path_factory.mktemp("exact_ref")), **R.PROBLEM_A)
    vs = [X.smooth_v(pb, 3), X.smooth_v(pb, 4), X.white_v(pb, 5)]
    return pb, vs, [X.jv_ref(oracle, pb, v) for v in vs]


def test_omega_is_the_interior_without_its_first_row_and_column(prob_a):
    pb, vs, _ = prob_a
    m = X.mask_omega(pb)
    nPml, nPad = pb["nPml"], pb["nPad"]
    assert m.sum() == (pb["nz_pad"] - nPad - 2 * nPml - 1) * (pb["nx_pad"] - 2 * nPml - 1)
    assert m[nPml + 1, nPml + 1] and not m[nPml, nPml + 1] and not m[nPml + 1, nPml] and m[pb["nz_pad"] - nPad - nPml - 1, pb["nx_pad"] - nPml - 1]
    assert all(np.abs(a[m]).max() > 0 and not np.any(a[~m]) for v in vs for a in v)
    assert all(m[z, x] for _, z, x in X.PROBE_CELLS)
    assert max(z for _, z, _ in X.PROBE_CELLS) <= nPml + 30


def test_the_pairs_of_the_gpu_tests_are_neither_parallel_nor_orthogonal(prob_a):
    _, _, jv = prob_a
    for k, c in enumerate(X.COMPS):     # (printed: vz alone is not a pair any GPU test uses)
        print("cos(J v1, J v2), %s alone: %.3f" % (c, X.cosine(jv[0], jv[1], [float(j == k) for j in range(3)])))
    for weights in X.WEIGHTS:
        cos = X.cosine(jv[0], jv[1], weights)
        print("cos(W^1/2 J v1, W^1/2 J v2), weights %r: %.3f" % (weights, cos))
        assert 0.1 <= abs(cos) <= 0.9, (weights, cos)


def test_the_reference_adjoint_misses_the_norm_by_more_than_the_tolerance(oracle, prob_a):
    """the oracle's gradient at obs = syn - J v, v masked to Omega, against |J v|^2: what a re-exported backward pass would give"""
    pb, vs, _ = prob_a
    b = dict(G=0, vertical=False, weights=None)
    m = [t.numpy() for t in pb["lame_init"]]
    syn, dsyn, _ = born_side(oracle, pb, pb["survey"], b, m, vs[0])
    ref = shifted_gradient(oracle, pb, pb["survey"], b, m, syn, dsyn)
    vhv = X.model_dot(vs[0], [ref[k] for k in GRADS])
    miss = abs(vhv / ref["jv2"] - 1.0)
    print("the reference's adjoint on v masked to Omega: v^T H v / |J v|^2 = %.5f (misses by %.2e)" % (vhv / ref["jv2"], miss))
    assert miss >= 5.0 * X.TOL, miss


def test_probe_cells_are_reached_by_the_wave(oracle, prob_a):
    pb, _, _ = prob_a
    norms = []
    for param in range(3):
        scale = 0.01 * float(np.abs(pb["lame_init"][param].numpy()).mean())
        norms.append(X.probe_dots(oracle, pb, param, X.PROBE_CELLS, None, scale=scale, norms=True))
        print("|J e_k| of parameter %d at the probe cells: %s" % (param, " ".join("%.2e" % n for n in norms[-1])))
        assert np.all(norms[-1] > 1e-6 * norms[-1].max()), (param, norms[-1])
    far = X.probe_dots(oracle, pb, 0, [(0, 59, 99)], None, scale=0.01 * float(np.abs(pb["lame_init"][0].numpy()).mean()), norms=True)[0]
    print("|J e_k| in the far corner (59, 99): %.2e" % far)
    assert far < 1e-6 * norms[0].max()


def test_symbol_is_exported_and_refusals_need_no_device():
    from sepfwi import _native
    L = _native.lib()
    assert "sepfwi_adjoint_exact" in _native.EXPORTS and hasattr(L, "sepfwi_adjoint_exact")
    hdr = open(os.path.join(ROOT, "include", "sepfwi.h")).read()
    assert "int sepfwi_adjoint_exact(float *misfit, float *g_Lambda, float *g_Mu, float *g_Den, const float *w_ett" in hdr
    a = np.zeros(4, np.float32)
    ids = np.zeros(1, np.int32)
    p, ip, fn = C.c_void_p(a.ctypes.data), C.c_void_p(ids.ctypes.data), b"/nonexistent/para.json"
    call = lambda *args: L.sepfwi_adjoint_exact(*args, 0, 1, ip, fn, None)
    #            misfit g_L g_M g_D    w_ett w_vx w_vz    dL dM dD     L M D stf
    assert call(None, p, None, p, None, None, None, None, None, None, p, p, p, p) == -1 and b"g_" in L.sepfwi_last_error()
    assert call(None, p, p, p, None, None, None, None, None, None, p, None, p, p) == -1 and b"must not be NULL" in L.sepfwi_last_error()
    assert call(None, p, p, p, None, None, None, p, None, p, p, p, p, p) == -1 and b"all NULL or all set" in L.sepfwi_last_error()
    assert call(None, p, p, p, p, None, None, p, p, p, p, p, p, p) == -1 and b"not both" in L.sepfwi_last_error()
    assert L.sepfwi_adjoint_exact(None, p, p, p, p, None, None, None, None, None, p, p, p, p, 0, 1, None, fn, None) == -1 and b"shot list" in L.sepfwi_last_error()
    assert L.sepfwi_adjoint_exact(None, p, p, p, p, None, None, None, None, None, p, p, p, p, 0, 1, ip, None, None) == -1


def test_header_with_the_new_function_is_valid_c_and_cpp(tmp_path):
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no host compiler")
    inc = os.path.join(ROOT, "include")
    body = ('#include "sepfwi.h"\nint f(float *g, const float *w, const float *m, const int *ids) {\n'
            '    return sepfwi_adjoint_exact(0, g, g, g, w, 0, 0, 0, 0, 0, m, m, m, m, 0, 1, ids, "p.json", 0);\n}\n')
    c = tmp_path / "t.c"
    c.write_text(body)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", inc, str(c)])
    cpp = tmp_path / "t.cpp"
    cpp.write_text(body)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, str(cpp)])
