"""The reference side of tests/test_gpu_param_chain_fuzz.py on its default 16 seeds, on the CPU (tests/param_tangent_ref.py: draw_grid,
fuzz_inputs, diag_ref64, settled_inputs): what the generators draw is held by a digest; between them the draws hold the paths of
k_param_bwd_rim / k_param_diag_rim that the fixed grids of tests/test_gpu_param_tangent.py leave out; the float64 `diag` reference for
any size equals the dense Jacobian's on the tiny grids; every default seed x class has a target, so none reaches the xfail branch on the
GPU; and the comparison can fail: two host restatements of a wrong rim sum miss the reference by at least 5 x the bound.

Measured here (float32 torch path against the float64 references, largest over tangent / pullback / diag and the arrays, at the attempt
that settled_inputs takes): algebraic kinds up to 4.9e-7 of the 6.7e-7 that a third of their bound is, rock physics up to 6.6e-7 of the
6.7e-7 that two thirds of theirs is (target_share); 100 of the 112 draws take attempt 0, six attempt 1, four attempt 2, two attempt 4.
The two wrong rim sums miss `diag` by 0.49 ... 0.70 and 0.92 ... 1.0 of its maximum."""
import hashlib

import numpy as np
import pytest
import torch

import param_tangent_ref as T

SEEDS = T.DEFAULT_SEEDS
DRAWS_DIGEST = "645400b876230a63c32e2613997baa861ae6e41036f8a3245977918d8a1570c6"


def _modules64(cls_name, seed, attempt=0):
    dims, mask_kind, f, mask, v, w, h = T.fuzz_inputs(cls_name, seed, attempt)
    return dims, mask, h, T.make_module(cls_name, dims, f, mask, dtype=torch.float64)


def test_param_chain_fuzz_draws_are_what_they_were():
    """Grid, kind of mask and every array of attempt 0, for the 16 default seeds and the seven classes."""
    hh = hashlib.sha256()
    for seed in SEEDS:
        for cls_name in T.CLASSES:
            dims, mask_kind, f, mask, v, w, h = T.fuzz_inputs(cls_name, seed)
            assert dims == T.draw_grid(seed) and mask.shape == T.padded_shape(dims)
            hh.update(repr((seed, cls_name, dims, mask_kind)).encode())
            for a in [np.asarray(x, np.float32) for x in f] + [mask] + v + w + h:
                assert a.dtype == np.float32
                hh.update(np.ascontiguousarray(a).tobytes())
    assert hh.hexdigest() == DRAWS_DIGEST


def test_param_chain_fuzz_draws_cover_what_the_fuzz_is_for():
    count = {k: 0 for k in ("one row", "one column", "two rows", "nPad without nPml", "three passes", "long strip", "deep strip")}
    widths, masks, rim_masks = set(), {k: 0 for k in T.MASK_KINDS}, {}
    for seed in SEEDS:
        nz, nx, nPml, nPad = dims = T.draw_grid(seed)
        nzp, nxp = T.padded_shape(dims)
        mask_kind, mask = T.fuzz_inputs("FWI", seed)[1], T.fuzz_inputs("FWI", seed)[3]
        print("param chain fuzz seed %2d: %-18s %r padded %d x %d, mask %s" % (seed, T.GRID_KINDS[seed % len(T.GRID_KINDS)], dims, nzp, nxp, mask_kind))
        assert nz >= 1 and nx >= 1 and nzp * nxp <= 40 * 129
        masks[mask_kind] += 1
        pad = np.ones((nzp, nxp), bool)
        pad[nPml:nPml + nz, nPml:nPml + nx] = False
        if mask_kind == "fractional padding":
            assert pad.any() and np.all((mask[pad] > 0) & (mask[pad] < 1)) and np.all(mask[~pad] == 1)
        live = bool(np.any(mask[pad] != 0))      # the rim sums are not switched off
        if nx > 3:
            widths.add(nxp)
            assert 3 <= nz <= 9 and nzp % 4 != 0, dims
            continue
        assert nz <= 3 and nx <= 3 and nPml <= 12, dims
        for name, on in (("one row", nz == 1 and nx > 1 and nPml > 0), ("one column", nx == 1 and nz > 2 and nPml > 0), ("two rows", nz == 2),
                         ("nPad without nPml", nPml == 0 and nPad > 0), ("three passes", (nPml + 1) ** 2 > 128),
                         ("long strip", nPml + nPad + 1 > 64 and nx >= 3), ("deep strip", nPml >= 8 and nPad > 0)):
            count[name] += bool(on)
            rim_masks[name] = rim_masks.get(name, False) or (bool(on) and live)
    print(count, sorted(widths), masks)
    assert all(n >= 1 for n in count.values()), count
    assert all(rim_masks[k] for k in ("one row", "one column", "three passes", "long strip", "deep strip")), rim_masks
    assert widths == set(T.WIDTHS), widths
    assert all(n >= 2 for n in masks.values()), masks


@pytest.mark.parametrize("seed", [s for s in SEEDS if T.draw_grid(s)[1] <= 3])
def test_diag_reference_is_the_dense_jacobian_s_on_the_tiny_grids(seed):
    """diag_ref64 (three jvps and E^T by autograd) against diag64 (dense Jacobian) to 1e-12, for an algebraic kind and a rock-physics map
    per tiny draw, going round the classes with the seed; and rim_sum_restated without a defect is E^T."""
    for cls_name in (T.CLASSES[seed % 5], T.CLASSES[5 + seed % 2]):
        dims, mask, h, m64 = _modules64(cls_name, seed)
        ref, dense = T.diag_ref64(m64, h), T.diag64(m64, h)
        devs = T.deviations(ref, dense)
        print("param chain fuzz seed %d %s %r: diag_ref64 against the dense Jacobian %s" % (seed, cls_name, dims, ["%.1e" % d for d in devs]))
        assert all(a.shape == dims[:2] and np.abs(b).max() > 0 for a, b in zip(ref, dense)) and max(devs) <= 1e-12
        assert max(T.deviations(T.rim_sum_restated(T.cell_terms64(m64, h), dims), dense)) <= 1e-12


def test_every_default_draw_has_a_target():
    """The float32 torch path (tangent, pullback, diag) within target_share of the bound at one of the attempts, for all 16 x 7."""
    taken = []
    for seed in SEEDS:
        for cls_name in T.CLASSES:
            o, attempt = T.settled_inputs(cls_name, seed)
            assert o is not None, (seed, cls_name, T.float32_path(cls_name, seed))
            p = T.float32_path(cls_name, seed, attempt)
            print("param chain fuzz seed %2d %-26s attempt %d: float32 torch path %s (target %.1e)"
                  % (seed, cls_name, attempt, {k: "%.1e" % max(d) for k, d in p.items()}, T.target_share(cls_name) * T.tol_of(cls_name)))
            taken.append(attempt)
    print("attempts taken:", [taken.count(k) for k in range(T.ATTEMPTS)])


def test_a_wrong_rim_sum_misses_the_reference():
    """The comparison can fail.  "Only the first 64 replicas are summed" (the lane loop reduced to its first pass) against diag64 on the
    draw whose corner rectangles hold more than 128 cells, and "a one-row grid counted twice" (the nz == 1 guard removed) on the one-row
    draws: the rim part doubles."""
    seen = dict(first=0, twice=0)
    for seed in SEEDS:
        nz, nx, nPml, nPad = dims = T.draw_grid(seed)
        first, twice = nx <= 3 and (nPml + 1) ** 2 > 64, nz == 1
        if not (first or twice):
            continue
        for cls_name in T.CLASSES:
            dims, mask, h, m64 = _modules64(cls_name, seed)
            dense, cells = T.diag64(m64, h), T.cell_terms64(m64, h)
            if first:
                dev = max(T.deviations(T.rim_sum_restated(cells, dims, passes=1), dense))
                print("param chain fuzz seed %d %s %r: the first pass alone misses diag by %.2e of the maximum" % (seed, cls_name, dims, dev))
                assert dev >= 5.0 * T.tol_of(cls_name)
                seen["first"] += 1
            if twice:
                wrong = T.rim_sum_restated(cells, dims, one_row_twice=True)
                own = [c[nPml:nPml + nz, nPml:nPml + nx] for c in cells]
                ratio = [float(((a - o) / (d - o)).min()) for a, d, o in zip(wrong, dense, own)]
                dev = max(T.deviations(wrong, dense))
                print("param chain fuzz seed %d %s %r: the rim of a one-row grid counted twice: rim part x %s, diag off by %.2e of the maximum"
                      % (seed, cls_name, dims, ["%.3f" % r for r in ratio], dev))
                assert all(abs(r - 2.0) <= 1e-9 for r in ratio) and dev >= 5.0 * T.tol_of(cls_name)
                seen["twice"] += 1
    assert seen["first"] >= 7 and seen["twice"] >= 7, seen
