"""The reference that the Born-modelling GPU tests rest on (tests/born_ref.py), checked on the CPU: its background loop IS the oracle's
forward loop (same gathers, bit for bit), it is linear in v, and its scattered gathers are the derivative of the oracle's gathers --
central finite differences (d(m + eps v) - d(m - eps v)) / 2 eps of oracle.cufd(calc_id 2) over a decade ladder of eps.

Measured (rel-L2 against the finite difference per component [pr, vx, vz, ett], best eps of the ladder; float32 oracle):
  problem A (50 x 90, heterogeneous)     joint v 1.3e-4 1.4e-4 1.5e-4 2.7e-4 | dLambda 5.9e-5 7.6e-5 6.9e-5 1.9e-4
                                         dMu     7.4e-5 1.5e-4 9.8e-5 2.0e-4 | dDen    1.4e-4 1.6e-4 1.6e-4 2.0e-4
  problem W (the same with 22 rows of water: mu = 0)
                                         joint v 1.2e-4 1.0e-4 8.8e-5 1.7e-4 | dLambda 1.6e-4 1.2e-4 1.1e-4 2.2e-4
                                         dMu     1.3e-4 9.1e-5 1.1e-4 1.6e-4 | dDen    2.3e-4 2.0e-4 1.5e-4 3.6e-4
The curve is the textbook one: truncation ~ eps^2 above the minimum (1.7e-2 at eps 10, 1.7e-4 at eps 1 on A), round-off ~ 1 / eps
below it (1.4e-3 at 0.01, 1.4e-2 at 0.001).  All far below 1e-2, while a dropped coupling term is an error of 0.35 ... 1.0 (asserted
below), so the check discriminates.  Linearity born(2 v) against 2 born(v): worst deviation 4.8e-7 of a component's maximum."""
import numpy as np
import pytest

import born_ref as B
import oracle_loop as OL
import problems as P

COMPS = ("pr", "vx", "vz", "ett")
LADDER = (10.0, 1.0, 0.1, 0.01, 0.001)
# best-of-ladder rel-L2 per component as measured (module docstring): {(problem, only): [pr, vx, vz, ett]}
MEASURED = {
    ("A", None): [1.32e-4, 1.42e-4, 1.47e-4, 2.66e-4], ("A", 0): [5.85e-5, 7.62e-5, 6.90e-5, 1.85e-4],
    ("A", 1): [7.37e-5, 1.51e-4, 9.82e-5, 1.98e-4], ("A", 2): [1.39e-4, 1.57e-4, 1.61e-4, 1.96e-4],
    ("W", None): [1.18e-4, 1.02e-4, 8.80e-5, 1.73e-4], ("W", 0): [1.64e-4, 1.16e-4, 1.13e-4, 2.16e-4],
    ("W", 1): [1.25e-4, 9.05e-5, 1.11e-4, 1.61e-4], ("W", 2): [2.32e-4, 1.96e-4, 1.45e-4, 3.61e-4],
}
LINEARITY_MEASURED = 4.8e-7


@pytest.fixture(scope="module")
def setups(oracle, tmp_path_factory):
    out = {}
    for name in ("A", "W"):
        pb, w = B.water_problem(tmp_path_factory.mktemp("born_" + name), name)
        m = [t.numpy() for t in pb["lame_init"]]
        rest = (pb["Stf"].numpy(), pb["Shot_ids"].numpy(), pb["para"], pb["survey"])
        out[name] = dict(pb=pb, w=w, m=m, rest=rest, v=B.perturbation(pb, water_rows=w))
        out[name]["ref"] = B.born(oracle, *m, *out[name]["v"], *rest)
    return out


@pytest.mark.parametrize("name", ["A", "W"])
def test_background_is_the_oracle_s_forward_loop(oracle, setups, name):
    s = setups[name]
    plain = oracle.cufd(*s["m"], s["rest"][0], 2, *s["rest"][1:])["syn"]
    assert np.abs(plain).max() > 0 and np.abs(s["ref"]["dsyn"]).max() > 0
    assert np.array_equal(s["ref"]["syn"], plain)


@pytest.mark.parametrize("name", ["A", "W"])
def test_linear_in_v(oracle, setups, name):
    s = setups[name]
    twice = B.born(oracle, *s["m"], *[2.0 * a for a in s["v"]], *s["rest"])["dsyn"]
    dev = [float(np.abs(twice[:, k] - 2.0 * s["ref"]["dsyn"][:, k]).max() / np.abs(2.0 * s["ref"]["dsyn"][:, k]).max()) for k in range(4)]
    print("born_ref %s: born(2v) against 2 born(v), worst deviation / max per component %s" % (name, ["%.2e" % d for d in dev]))
    assert max(dev) <= 4.0 * LINEARITY_MEASURED


def fd_ladder(oracle, s, v, ladder):
    """{eps: central finite difference of the oracle's gathers, float64}"""
    out = {}
    for eps in ladder:
        e = np.float32(eps)
        p = oracle.cufd(*[a + e * b for a, b in zip(s["m"], v)], s["rest"][0], 2, *s["rest"][1:])["syn"].astype(np.float64)
        q = oracle.cufd(*[a - e * b for a, b in zip(s["m"], v)], s["rest"][0], 2, *s["rest"][1:])["syn"].astype(np.float64)
        out[eps] = (p - q) / (2.0 * eps)
    return out


@pytest.mark.parametrize("only", [None, 0, 1, 2])
@pytest.mark.parametrize("name", ["A", "W"])
def test_scattered_gathers_are_the_derivative_of_the_oracle_s(oracle, setups, name, only):
    s = setups[name]
    v = s["v"] if only is None else B.perturbation(s["pb"], only=only, water_rows=s["w"])
    ref = s["ref"]["dsyn"] if only is None else B.born(oracle, *s["m"], *v, *s["rest"])["dsyn"]
    fd = fd_ladder(oracle, s, v, LADDER if only is None else LADDER[1:4])
    best = []
    for k, c in enumerate(COMPS):
        errs = {eps: P.rel_l2(ref[:, k], d[:, k]) for eps, d in fd.items()}
        print("born_ref %s v %s %s: rel-L2 against the finite difference %s" % (name, "joint" if only is None else "dLambda dMu dDen".split()[only], c,
                                                                              {eps: "%.2e" % e for eps, e in errs.items()}))
        best.append(min(errs.values()))
    for k, c in enumerate(COMPS):
        rec = MEASURED[(name, only)][k]
        assert rec < 1e-2
        assert best[k] <= 3.0 * rec, (name, only, c, best[k], rec)      # 3 x: the ragged minimum of a float32 finite-difference curve


@pytest.mark.parametrize("only,terms", [(0, (False, True, True)), (1, (False, True, True)), (1, (True, False, True)), (2, (True, True, False))])
def test_a_dropped_coupling_term_is_an_order_one_error(oracle, setups, only, terms):
    """What the finite-difference check must be able to see: without the (lam, mu) / averaged-mu / density term of the parameter's own
    perturbation the gathers are wrong by 0.35 ... 1.0, thousands of times the finite-difference agreement above."""
    s = setups["A"]
    v = B.perturbation(s["pb"], only=only, water_rows=s["w"])
    full = B.born(oracle, *s["m"], *v, *s["rest"])["dsyn"]
    cut = B.born(oracle, *s["m"], *v, *s["rest"], terms=terms)["dsyn"]
    for k in range(4):
        assert P.rel_l2(cut[:, k], full[:, k]) > 0.3, (only, terms, COMPS[k])


@pytest.mark.parametrize("name", ["A", "W"])
def test_perturbed_media_are_the_derivative_of_the_oracle_s_averages(oracle, setups, name):
    """Each of the five arrays against a central difference of the oracle's own media at m +- v (v is 1 % of the model: truncation
    ~ 1e-4 of the derivative, float32 round-off of the averages 1e-7 / 1e-2 = 1e-5), float64 differences.  Bound 1e-3."""
    s = setups[name]
    pb = s["pb"]
    nz, nx = pb["nz_pad"], pb["nx_pad"]
    hi = OL.internal_media(oracle, *[a + b for a, b in zip(s["m"], s["v"])], nz, nx)
    lo = OL.internal_media(oracle, *[a - b for a, b in zip(s["m"], s["v"])], nz, nx)
    fd = {k: (hi[j].astype(np.float64) - lo[j].astype(np.float64)) / 2.0 for k, j in (("dlam", 0), ("dmu", 1), ("damu", 3), ("dba", 4), ("dbb", 5))}
    for k, got in zip(("dlam", "dmu", "damu", "dba", "dbb"), s["ref"]["dmedia"]):
        err = P.rel_l2(got, fd[k])
        print("born_ref %s: %s against the finite difference of the oracle's media, rel-L2 %.2e" % (name, k, err))
        assert np.abs(fd[k]).max() > 0 and err <= 1e-3, (k, err)
        edge = np.ones((nx, nz), bool)
        edge[2:nx - 2, 2:nz - 2] = False
        if k in ("damu", "dba", "dbb"):
            assert (got[edge] == 0).all(), k
    if s["w"]:      # water: the averaged mu and its derivative are 0 wherever one of the four cells is a fluid
        assert (s["ref"]["dmedia"][2][:, :s["w"]] == 0).all()
