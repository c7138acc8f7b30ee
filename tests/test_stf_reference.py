"""The source block's reference on the CPU (tests/stf_ref.py; csrc/born.hpp and csrc/exact_adjoint.hpp "Source block"): the oracle is
linear in the source time function, which licenses js_ref (J_s ds = the oracle's gathers with stf = ds); the end taper of the source
rows is a pointwise window (its transpose is itself, a tapered trace of ones); the two entry points are declared, exported and refuse
what include/sepfwi.h says they refuse before a device is needed; and the default seeds of tests/test_gpu_source_adjoint_fuzz.py have a
live record and a target on the oracle side alone, so at most a quarter of them (in fact none) can reach that test's xfail branch."""
import ctypes as C
import os

import numpy as np
import pytest

import fuzz_common as FC
import fuzz_draws as D
import problems as P
import stf_ref as S
from born_ref import COMPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WATER_SEED = 0      # a default seed of the fuzz whose draw has a water layer (asserted below)


def _linearity(oracle, oracle_nvfma, model, stf, ids, para, sv, what):
    ds = S.draw_ds(1, stf)
    both = S.js_ref(oracle, model, stf + ds, ids, para, sv)
    base = S.js_ref(oracle, model, stf, ids, para, sv)
    lin, alt = S.js_ref(oracle, model, ds, ids, para, sv), S.js_ref(oracle_nvfma, model, ds, ids, para, sv)
    for i in range(len(lin)):
        for c in COMPS:
            a, r, r2 = both[i][c] - base[i][c], lin[i][c], alt[i][c]
            top = float(np.abs(r).max())
            assert top > 0, (what, i, c)
            dev_max, dev_l2 = float(np.abs(a - r).max()), FC.d64(a, r)
            print("stf linearity %s, shot %d %s: max deviation %.2e of the peak, rel-L2 %.2e (the two oracle builds %.2e, %.2e)"
                  % (what, i, c, dev_max / top, dev_l2 / FC.l2(r), float(np.abs(r2 - r).max()) / top, FC.d64(r2, r) / FC.l2(r)))
            assert dev_max <= FC.GATHER_TOL * top + FC.YARD * float(np.abs(r2 - r).max()), (what, i, c)
            assert FC.array_held(a, r, r2, FC.GATHER_TOL), (what, i, c)


def test_the_oracle_is_linear_in_the_source(tmp_path, oracle, oracle_nvfma):
    """oracle(stf + ds) - oracle(stf) = oracle(ds) per shot and component: seismogram tolerance (1e-4 of the component's maximum, rel-L2
    1e-4) plus 3 x the two oracle builds' difference.  The default problem, and a fuzz draw with a water layer."""
    pb = P.make_problem(str(tmp_path / "default"))
    _linearity(oracle, oracle_nvfma, [t.numpy() for t in pb["lame_init"]], pb["Stf"].numpy(), pb["Shot_ids"].numpy(), pb["para"], pb["survey"], "default problem")
    d = D.draw_problem(tmp_path / "water", WATER_SEED, 1)
    assert d["water"] > 0, "seed %d no longer draws a water layer" % WATER_SEED
    pw = d["pb"]
    para = {k: v for k, v in pw["para"].items() if k not in ("if_win", "filter", "if_cross_misfit", "if_src_update")}      # (raw gathers)
    _linearity(oracle, oracle_nvfma, [t.numpy() for t in pw["lame_init"]], pw["Stf"].numpy(), pw["Shot_ids"].numpy(), para, d["sv"],
               "fuzz seed %d, %d rows of water" % (WATER_SEED, d["water"]))


def test_the_taper_is_a_pointwise_window():
    """sepfwi_stf_taper(ds) = ds x sepfwi_stf_taper(ones), bit for bit, at the suite's record lengths; the window is 0 at sample 0 only."""
    from sepfwi import _native
    L = _native.lib()
    for nt, dt in ((240, 1.0e-3), (120, 1.0e-3), (400, 2.5e-4), (2000, 5.0e-4), (37, 1.7e-3)):
        ones = np.ones(nt, np.float32)
        assert L.sepfwi_stf_taper(C.c_void_p(ones.ctypes.data), nt, dt, 0.001) == 0
        for seed in (0, 1):
            ds = S.draw_ds(seed, np.ones((1, nt), np.float32))[0]
            got = ds.copy()
            assert L.sepfwi_stf_taper(C.c_void_p(got.ctypes.data), nt, dt, 0.001) == 0
            assert np.array_equal(got, ds * ones), (nt, dt)
        assert ones[0] == 0.0 and np.all(ones[1:] > 0.0) and np.all(ones <= 1.0), (nt, ones[:3], ones[-3:])


def test_symbols_are_declared_and_exported():
    from sepfwi import _native
    L = _native.lib()
    hdr = open(os.path.join(ROOT, "include", "sepfwi.h")).read()
    for name in ("sepfwi_born_src", "sepfwi_adjoint_exact_src"):
        assert name in _native.EXPORTS and hasattr(L, name), name
    assert "int sepfwi_born_src(float *d_ett, float *d_vx, float *d_vz, float *hv_Lambda" in hdr and "void *hip_stream, const float *dStf);" in hdr
    assert "int sepfwi_adjoint_exact_src(float *misfit, float *g_Lambda" in hdr and "const float *dStf, float *g_stf);" in hdr
    assert len(L.sepfwi_born_src.argtypes) == len(L.sepfwi_born.argtypes) + 1
    assert len(L.sepfwi_adjoint_exact_src.argtypes) == len(L.sepfwi_adjoint_exact.argtypes) + 2


def test_refusals_need_no_device():
    """The argument combinations include/sepfwi.h refuses, each SEPFWI_EINVAL with a message, before a session (a device) is asked for."""
    from sepfwi import _native
    L = _native.lib()
    a = np.zeros(4, np.float32)
    ids = np.zeros(1, np.int32)
    p, ip, fn = C.c_void_p(a.ctypes.data), C.c_void_p(ids.ctypes.data), b"/nonexistent/para.json"
    N = None
    # sepfwi_adjoint_exact_src(misfit, g x 3, w x 3, v x 3, model x 3, stf, gpu, n, ids, fname, stream, dStf, g_stf)
    ex = lambda w, v, dstf, gstf=p: L.sepfwi_adjoint_exact_src(N, p, p, p, *w, *v, p, p, p, p, 0, 1, ip, fn, N, dstf, gstf)
    assert ex((p, N, N), (N, N, N), p) == -1 and b"not both" in L.sepfwi_last_error() and b"dStf" in L.sepfwi_last_error()
    assert ex((N, N, p), (N, N, N), p, N) == -1 and b"not both" in L.sepfwi_last_error()
    assert ex((N, N, N), (p, N, p), p) == -1 and b"all NULL or all set" in L.sepfwi_last_error()
    assert ex((N, N, N), (N, p, N), N) == -1 and b"all NULL or all set" in L.sepfwi_last_error()
    assert ex((p, N, N), (p, p, p), N) == -1 and b"not both" in L.sepfwi_last_error()
    assert L.sepfwi_adjoint_exact_src(N, p, N, p, N, N, N, N, N, N, p, p, p, p, 0, 1, ip, fn, N, p, p) == -1 and b"g_" in L.sepfwi_last_error()
    assert L.sepfwi_adjoint_exact_src(N, p, p, p, N, N, N, N, N, N, p, p, p, p, 0, 1, N, fn, N, p, p) == -1 and b"shot list" in L.sepfwi_last_error()
    # the legal combinations get as far as the parameter file: all-NULL v with dStf (the product), nothing at all (the gradient mode)
    for dstf in (p, N):
        rc, msg = ex((N, N, N), (N, N, N), dstf), L.sepfwi_last_error()
        assert rc != 0 and b"not both" not in msg and b"all NULL" not in msg, (rc, msg)
    # sepfwi_born_src(d x 3, hv x 3, model x 3, v x 3, stf, gpu, n, ids, fname, stream, dStf)
    bo = lambda hv, v, dstf: L.sepfwi_born_src(p, N, N, *hv, p, p, p, *v, p, 0, 1, ip, fn, N, dstf)
    assert bo((N, N, N), (p, N, p), p) == -1 and b"all NULL or all set" in L.sepfwi_last_error()
    assert bo((N, N, N), (N, N, N), N) == -1 and b"must not be NULL" in L.sepfwi_last_error()
    assert bo((N, N, N), (p, N, p), N) == -1 and b"must not be NULL" in L.sepfwi_last_error()
    assert bo((p, p, p), (p, p, p), p) == -1 and b"exact adjoint" in L.sepfwi_last_error()
    assert bo((p, N, N), (p, p, p), p) == -1 and b"all NULL (J v only) or all set" in L.sepfwi_last_error()
    rc, msg = bo((N, N, N), (N, N, N), p), L.sepfwi_last_error()      # legal: it gets as far as the parameter file
    assert rc != 0 and b"all NULL" not in msg and b"must not be NULL" not in msg, (rc, msg)


@pytest.fixture(scope="module")
def sides(oracle, oracle_nvfma, tmp_path_factory):
    return FC.default_sides(S.source_oracle_side, tmp_path_factory.mktemp("source_fuzz"), oracle, oracle_nvfma)


def test_source_fuzz_default_seeds_have_targets(sides):
    """The oracle side of the source fuzz on its default seeds: how many would be reported instead of compared (no live record at any
    scale, or a yardstick above 1e-2 of its scale) -- at most a quarter; and between them the draws hold channels inside the absorbing
    strips, ragged counts, joint weights, a gauge and a water layer."""
    skipped, count = [], dict(layer=0, ragged=0, weights=0, gauge=0, water=0)
    for seed in FC.DEFAULT_SEEDS:
        o, scale = sides[seed]
        if o is None or not o["target"]:
            skipped.append(seed)
            continue
        src = o["src"]
        print("source fuzz seed %d (scale %d): build spread %r; |J_s ds|^2 / |J_m v|^2 = %.2e"
              % (seed, scale, {k: "%.1e" % y for k, y in src["yard"].items()}, src["ref"]["n_s1"] / o["ref"]["nv"]))
        for ds in (src["ds1"], src["ds2"]):
            assert ds.shape == tuple(o["d"]["pb"]["Stf"].shape) and np.all(ds[:, 0] != 0) and np.all(ds[:, -1] != 0), seed
        for name, on in (("layer", o["e"]["layer"]), ("ragged", o["b"]["ragged"]), ("weights", o["b"]["weights"]), ("gauge", o["b"]["G"]), ("water", o["d"]["water"])):
            count[name] += bool(on)
    print("source fuzz: skipped seeds %r; %r" % (skipped, count))
    assert 4 * len(skipped) <= len(FC.DEFAULT_SEEDS), skipped
    assert all(v >= 1 for v in count.values()), count
