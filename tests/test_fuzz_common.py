"""The yardstick predicates of tests/fuzz_common.py on made-up numbers (pure numpy): a deviation of 0.99 times the bound passes and one of
1.01 times fails, with and without a difference between the two builds; an error confined to the rows below the water fails although
the whole image's bound would pass it; the cap sits at 1e-2.  A wrong sign, a dropped factor 3 or a norm over the wrong array fails here."""
import numpy as np
import pytest

import fuzz_common as C

NOMINAL, COND, SPREAD = 1e-3, 2.5e-4, 3e-4


def _vectors(builds_differ=True):
    """ref, a direction u with |u| = |ref|, and a second build SPREAD |ref| away from ref (or ref itself)"""
    rng = np.random.default_rng(20)
    ref, u, n = rng.standard_normal((3, 40, 30))
    return ref, u * (C.l2(ref) / C.l2(u)), ref + (SPREAD * C.l2(ref) / C.l2(n)) * n if builds_differ else ref


@pytest.mark.parametrize("builds_differ", [False, True])
@pytest.mark.parametrize("dist", [C.d64, C.d_own])
def test_array_and_gradient_hold_just_inside_the_bound_and_not_just_outside(builds_differ, dist):
    ref, u, alt = _vectors(builds_differ)
    bound = (NOMINAL + COND) + C.YARD * (SPREAD if builds_differ else 0.0)      # relative to |ref|
    inside, outside = ref + 0.99 * bound * u, ref + 1.01 * bound * u
    assert C.array_held(inside, ref, alt, NOMINAL, COND, dist) and not C.array_held(outside, ref, alt, NOMINAL, COND, dist)
    assert C.gradient_miss(inside, ref, alt, NOMINAL, COND, 0, dist) == ""
    assert C.gradient_miss(outside, ref, alt, NOMINAL, COND, 0, dist) == "the whole image"
    assert not C.array_held(ref + 1.01 * NOMINAL * u, ref, ref, NOMINAL, 0.0, dist)      # no conditioning term, no spread: the nominal bound


@pytest.mark.parametrize("builds_differ", [False, True])
def test_scalar_holds_just_inside_the_bound_and_not_just_outside(builds_differ):
    ref, scale, floor = -7.25, 40.0, 1e-3
    alt = ref + (2e-3 if builds_differ else 0.0)
    own = (NOMINAL + COND) * abs(ref) + C.YARD * abs(alt - ref) + floor
    given = NOMINAL * scale + C.YARD * abs(alt - ref)
    for sign in (1.0, -1.0):
        assert C.scalar_held(ref + sign * 0.99 * own, ref, alt, NOMINAL, None, COND, floor)
        assert not C.scalar_held(ref + sign * 1.01 * own, ref, alt, NOMINAL, None, COND, floor)
        assert C.scalar_held(ref + sign * 0.99 * given, ref, alt, NOMINAL, scale) and not C.scalar_held(ref + sign * 1.01 * given, ref, alt, NOMINAL, scale)
    assert not C.scalar_held(float("nan"), ref, alt, NOMINAL)


def test_an_error_confined_to_the_rows_below_the_water_fails_on_its_own():
    """The image below 25 rows of water is 1e-2 of the whole, so the floor of 3 % of the whole image's norm decides there.  An error of
    half the whole image's bound, all of it below the water, passes as a whole and must fail below the water; so must it when the two
    builds differ above the water only."""
    ref, u, _ = _vectors()
    water = 25
    ref[water:] *= 1e-2 * C.l2(ref[:water]) / C.l2(ref[water:])
    e = np.zeros_like(ref)
    e[water:] = u[water:]
    e *= NOMINAL * C.l2(ref) / C.l2(e)      # |e| = the whole image's bound
    alt = ref.copy()
    alt[:water] += 1e-3 * u[:water]
    for other in (ref, alt):
        assert C.array_held(ref + 0.5 * e, ref, other, NOMINAL) and C.gradient_miss(ref + 0.5 * e, ref, other, NOMINAL, 0.0, 0) == ""
        assert C.gradient_miss(ref + 0.5 * e, ref, other, NOMINAL, 0.0, water) == "below the water"
    assert C.gradient_miss(ref + 0.99 * C.WATER_FLOOR * e, ref, ref, NOMINAL, 0.0, water) == ""
    assert C.gradient_miss(ref + 1.01 * C.WATER_FLOOR * e, ref, ref, NOMINAL, 0.0, water) == "below the water"


def test_the_cap_and_the_constants():
    assert C.has_target(0.99e-2, 0.99e-2) and not C.has_target(1.01e-2, 0.0) and not C.has_target(0.0, 1.01e-2)
    assert (C.GATHER_TOL, C.MISFIT_TOL, C.GRAD_TOL, C.STF_TOL, C.YARD, C.WATER_FLOOR, C.TARGET_CAP, C.PRECURSOR) == (1e-4, 1e-4, 1e-3, 5e-3, 3.0, 3e-2, 1e-2, 3e-10)
    E, m = 3.0e4, 1.2e-3
    assert C.conditioning(E, m) == (8.0 * 2.0 ** -24 * np.sqrt(m * E), 4.0 * 2.0 ** -24 * np.sqrt(E / m))
    assert C.is_precursor(2.9e-10 * 7.0, 7.0) and not C.is_precursor(3.1e-10 * 7.0, 7.0)
