"""The oracle side of tests/test_gpu_pseudo_hessian_fuzz.py, on the CPU: the definition in tests/pseudo_hessian_ref.py is licensed on
unequal spacings against the oracle's own stress and velocity kernels, and the default 16 seeds are compared on enough live cells.

THE DEFINITION.  pseudo_hessian_ref.combinations evaluates a, b, s, Fz, Fx in float64; nothing but the GPU kernel that restates them ever
checked their derivatives, and on dz == dx an exchanged spacing or a transposed axis changes nothing.  The oracle's forward kernels
compute the same eight derivatives on every interior cell (no interior cell takes a C-PML branch), so with unit media and zeroed targets
one call of oracle_loop.Setup.stress / velocity on smooth random fields leaves
    szz = sxx = dt (a + b)                        (Lambda = 1, Mu = 0)
    szz = 2 dt a,  sxx = 2 dt b,  sxz = dt s      (Lambda = 0, Mu = 1, the averaged Mu = 1)
    vz = dt Fz,  vx = dt Fx                       (both buoyancies 1)
in float32.  Bound, with u = 2^-24 the unit round-off of float32 and T the sum of the absolute stencil terms of the derivatives that enter
a value, T = sum over its derivatives of (c1 (|f0| + |f1|) + c2 (|f2| + |f3|)) / h:  a float32 derivative carries at most
1 u (its inner differences) + 1 u (c2 = fl(1/24); c1 is exact) + 1 u (the products) + 1 u (the outer difference) + 1 u (the division)
+ 1 u (h = fl(dz) in the kernel, the decimal dz in the reference) = 6 u of its T; the sum of two derivatives 1 u (float32 in sxz and
the velocities, float64 in szz, sxx); the factors 1 and 2 none; the multiply-add with dt and the store 2 u.  9 u T dt to first order;
the bound asserted is 10 u T dt.  The same evaluation with dz and dx EXCHANGED is an error of |dz / dx - 1| of a derivative and must miss
this bound by orders of magnitude -- asserted, so the test is known to see what it is for.

THE DRAWS.  Per default seed at its settled scale (fuzz_sides.pseudo_hessian_side: the first scale at which 90 % of the outermost
interior ring is live, E >= 1e-30): the live shares of the interior and of the ring, both at least the cap of 25 % below which the GPU
test fails a draw as not tested, and the per-cell spread between the two oracle builds on the live cells, the yardstick term of the
GPU test's bound."""
import numpy as np
import pytest

import fuzz_common as C
import fuzz_draws as D
import oracle_loop as OL
import problems as P
import pseudo_hessian_ref as R
from fuzz_sides import PH_CAP, PH_SETTLED, describe_pseudo_hessian, pseudo_hessian_side

SEEDS = C.DEFAULT_SEEDS
U = 2.0 ** -24
C1, C2 = R.C1, R.C2


def _abs_terms(f, kind, axis, xs, zs, h):
    """sum of the absolute stencil terms of one derivative, float64 on the interior block"""
    s = (lambda k: np.abs(R._shift(f, k, 0, xs, zs))) if axis == "x" else (lambda k: np.abs(R._shift(f, 0, k, xs, zs)))
    if kind == "-":
        return (C1 * (s(0) + s(-1)) + C2 * (s(1) + s(-2))) / h
    return (C1 * (s(1) + s(0)) + C2 * (s(2) + s(-1))) / h


def _terms(f, xs, zs, dz, dx):
    """T of the five combinations, in the order of pseudo_hessian_ref.combinations"""
    vz, vx, szz, sxx, sxz = [np.asarray(f[k], np.float64) for k in OL.FIELDS]
    return (_abs_terms(vz, "-", "z", xs, zs, dz), _abs_terms(vx, "-", "x", xs, zs, dx),
            _abs_terms(vx, "+", "z", xs, zs, dz) + _abs_terms(vz, "+", "x", xs, zs, dx),
            _abs_terms(szz, "+", "z", xs, zs, dz) + _abs_terms(sxz, "-", "x", xs, zs, dx),
            _abs_terms(sxz, "-", "z", xs, zs, dz) + _abs_terms(sxx, "+", "x", xs, zs, dx))


def _kernel_increments(s, f):
    """The five combinations times dt as the oracle build's own forward kernels compute them on the field set f: dict name -> [x][z]"""
    one, zero = np.ones((s.nx, s.nz), np.float32), np.zeros((s.nx, s.nz), np.float32)

    def run(kernel, media, inputs):
        g = s.new_fields()
        for k in inputs:
            g[k][...] = f[k]
        kernel(g, *media)
        return g

    lam = run(s.stress, (one, zero, zero), ("vz", "vx"))
    mu = run(s.stress, (zero, one, one), ("vz", "vx"))
    vel = run(s.velocity, (one, one), ("szz", "sxx", "sxz"))
    return {"a+b (szz)": lam["szz"], "a+b (sxx)": lam["sxx"], "2a": mu["szz"], "2b": mu["sxx"], "s": mu["sxz"], "Fz": vel["vz"], "Fx": vel["vx"]}


def _worst(s, f, got, dz, dx):
    """{name: the largest |kernel - dt * reference| / (u T dt) over the interior} for the reference evaluated with the spacings dz, dx"""
    xs, zs = slice(s.nPml, s.nx - s.nPml), slice(s.nPml, s.nzc - s.nPml)
    a, b, sh, Fz, Fx = R.combinations(f, xs, zs, dz, dx)
    Ta, Tb, Ts, Tz, Tx = _terms(f, xs, zs, s.dz, s.dx)
    dt = float(s.dtf)
    want = {"a+b (szz)": (a + b, Ta + Tb), "a+b (sxx)": (a + b, Ta + Tb), "2a": (2.0 * a, 2.0 * Ta), "2b": (2.0 * b, 2.0 * Tb), "s": (sh, Ts),
            "Fz": (Fz, Tz), "Fx": (Fx, Tx)}
    out = {}
    for name, (w, T) in want.items():
        g = got[name][xs, zs].astype(np.float64)
        assert np.isfinite(g).all() and np.abs(g).max() > 0 and T.min() > 0, name
        out[name] = float((np.abs(g - dt * w) / (U * T * dt)).max())
    return out


@pytest.mark.parametrize("build", ["unfused", "nvfma"])
def test_the_definition_is_the_oracle_s_own_kernels_on_unequal_spacings(oracle, oracle_nvfma, tmp_path, build):
    lib = oracle if build == "unfused" else oracle_nvfma
    for seed in SEEDS:      # the first default draw that is what the test needs: unequal spacings, a padded bottom, a grid that is not square
        pb = D.draw_problem(tmp_path / ("s%d" % seed), seed, 1)["pb"]
        s = OL.Setup(lib, *[t.numpy() for t in pb["lame_init"]], pb["para"])
        ratio = s.dz / s.dx
        if abs(ratio - 1.0) > 0.1 and s.nPad > 0 and s.nzc != s.nx:
            break
    else:
        raise AssertionError("no default draw with dz != dx and nPad > 0")
    rng = np.random.default_rng(4242)
    f = {k: OL.f32(P.smooth_random(rng, (s.nx, s.nz), -1.0, 1.0, passes=3)) for k in OL.FIELDS}
    got = _kernel_increments(s, f)
    right, swapped = _worst(s, f, got, s.dz, s.dx), _worst(s, f, got, s.dx, s.dz)
    print("pseudo-Hessian definition on the %s build, %d x %d nPml %d nPad %d dz/dx %.3f: |kernel - dt reference| / (u T dt) at most %s; with dz and dx exchanged %s"
          % (build, s.nz, s.nx, s.nPml, s.nPad, ratio, {k: "%.2f" % v for k, v in right.items()}, {k: "%.1e" % v for k, v in swapped.items()}))
    for name in right:
        assert right[name] <= 10.0, (name, right[name])
        assert swapped[name] > 10.0, (name, swapped[name])       # an exchanged spacing does not pass


@pytest.fixture(scope="module")
def sides(oracle, oracle_nvfma, tmp_path_factory):
    """{seed: (pseudo_hessian_side's dict, scale)} of the default seeds, with the re-draw of the GPU test"""
    return C.default_sides(pseudo_hessian_side, tmp_path_factory.mktemp("ph_fuzz"), oracle, oracle_nvfma)


def test_pseudo_hessian_fuzz_draws_are_compared_on_live_cells(sides):
    """NONE of the default seeds falls under the cap, the two builds agree per live cell far inside the nominal 1e-4, and between them
    the 16 draws hold what the fuzz is for."""
    seen, structures, worst = set(), set(), 0.0
    for seed in SEEDS:
        o, scale = sides[seed]
        assert o is not None, seed
        d, h, pb = o["d"], o["h"], o["d"]["pb"]
        inside, _ = R.masks(pb)
        spread = 0.0
        for name, ref, alt, live in zip(R.NAMES, o["ref"], o["alt"], R.live_cells(o["ref"], pb["para"]["dt"])):
            assert np.isfinite(ref).all() and (ref >= 0).all() and (ref[~inside] == 0).all() and (alt[~inside] == 0).all(), (seed, name)
            on = live & inside
            spread = max(spread, float((np.abs(alt[on] - ref[on]) / ref[on]).max()))
        worst = max(worst, spread)
        print("pseudo-Hessian fuzz seed %2d (%s): two-build spread per live cell %.1e" % (seed, describe_pseudo_hessian(o, scale), spread))
        assert o["interior"] >= PH_CAP and o["ring"] >= PH_CAP, (seed, o["interior"], o["ring"])
        assert o["ring"] >= PH_SETTLED or scale == C.SCALES[-1], (seed, scale, o["ring"])
        assert spread <= 1e-4 / 3.0, (seed, spread)      # the yardstick term 3 |alt - ref| stays below the nominal tolerance on every live cell
        structures.add(repr(h["opts"]))
        para = pb["para"]
        seen.update(name for name, on in (("dz != dx", para["dz"] != para["dx"]), ("nPad > 0", pb["nPad"] > 0), ("water", d["water"]), ("several shots", pb["Shot_ids"].numel() > 1),
                                          ("misfit call", h["entry"] == "forward"), ("gradient call", h["entry"] == "backward"), ("C ABI", h["fetch"] == "capi"),
                                          ("every > 1", h["every"] > 1), ("conditioned", d["extra"] in (2, 4, 5)), ("directional", d["extra"] == 1)) if on)
    print("worst two-build spread per live cell %.1e" % worst)
    want = {"dz != dx", "nPad > 0", "water", "several shots", "misfit call", "gradient call", "C ABI", "every > 1", "conditioned", "directional"}
    assert want <= seen, sorted(want - seen)
    assert len(structures) >= 6, structures
