"""The reference that the pseudo-Hessian GPU tests rest on (tests/pseudo_hessian_ref.py), checked on the CPU: its forward loop IS the
oracle's (same gathers, bit for bit), and what it accumulates has the properties of an illumination map -- finite, non-negative,
positive on the whole interior of the two test problems, exactly zero outside."""
import numpy as np
import pytest

import problems as P
import pseudo_hessian_ref as R


@pytest.fixture(scope="module")
def refs(oracle, tmp_path_factory):
    """Both problems through the reference once, every = 1 and 4: {name: (problem, {every: (hL, hM, hD)}, gathers)}."""
    out = {}
    for name, kw in (("A", R.PROBLEM_A), ("B", R.PROBLEM_B)):
        pb = P.make_problem(str(tmp_path_factory.mktemp("ph_" + name)), **kw)
        H, syn = R.pseudo_hessian(oracle, *[t.numpy() for t in pb["lame_init"]], pb["Stf"].numpy(), pb["Shot_ids"].numpy(), pb["para"],
                                  pb["survey"], every=(1, 4))
        out[name] = (pb, H, syn)
    return out


def test_reference_loop_is_the_oracle_s_forward_loop(oracle, refs):
    """The gathers of the restated loop equal oracle.cufd(..., calc_id 2) bit for bit: the accumulation sits in the oracle's own loop."""
    pb, _, syn = refs["A"]
    plain = oracle.cufd(*[t.numpy() for t in pb["lame_init"]], pb["Stf"].numpy(), 2, pb["Shot_ids"].numpy(), pb["para"], pb["survey"])["syn"]
    assert np.abs(plain).max() > 0
    assert np.array_equal(syn, plain)


@pytest.mark.parametrize("name", ["A", "B"])
def test_reference_is_an_illumination_map(refs, name):
    pb, H, _ = refs[name]
    nPml, nzc, nx = pb["nPml"], pb["nz_pad"] - pb["nPad"], pb["nx_pad"]
    inside = np.zeros((pb["nz_pad"], nx), bool)
    inside[nPml:nzc - nPml, nPml:nx - nPml] = True
    for k, h in zip(("hLambda", "hMu", "hDen"), H[1]):
        assert h.shape == inside.shape and np.isfinite(h).all() and (h >= 0).all(), k
        assert (h[inside] > 1e-6 * h.max()).all(), (k, h[inside].min() / h.max())     # every interior cell is illuminated
        assert (h[~inside] == 0).all(), k
    # sub-sampling in time is a quadrature of the same integral; recorded, not asserted (rel-L2 up to 7.7e-4 for rho on these problems)
    print("pseudo-Hessian reference %s: every = 4 against every = 1, rel-L2 %s" % (name, ["%.2e" % P.rel_l2(a, b) for a, b in zip(H[4], H[1])]))
