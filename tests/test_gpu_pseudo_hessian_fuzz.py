"""The diagonal pseudo-Hessian CELL BY CELL on random geometries and at the edges of its interior (-m gpu): csrc/pseudo_hessian.hip against
the float64 definition over the CPU oracle's forward loop (tests/pseudo_hessian_ref.py, licensed on dz != dx by
tests/test_pseudo_hessian_fuzz_reference.py).  tests/test_gpu_pseudo_hessian.py holds two fixed problems with dz == dx in the large; a norm over
the whole array does not see the outermost interior lines, which carry 1e-3 ... 1e-82 of it.

Every seed is a draw of tests/test_gpu_fuzz.py (fuzz_draws.draw_problem), unchanged, plus what fuzz_draws.draw_pseudo_hessian draws from a
generator of its own: the stride `every`, the entry point (a gradient call or a misfit-only call), one kernel-option set of the union of
OPTION_SETS and BORN_OPTION_SETS, and whether the result is the operator's return value or is fetched through the C ABI into host
memory.  The draw's conditioning keys, directional channels and water layer stay: the result may depend on none of them.  The record
is the first of fuzz_common.SCALES at which 90 % of the outermost interior ring is live (fuzz_sides.pseudo_hessian_side).

A cell is LIVE where the reference's un-scaled accumulator E = H / constant is at least 1e-30 (pseudo_hessian_ref.FLOOR).  Each value is a
sum of squares over time -- no cancellation -- so a cell-by-cell comparison is well conditioned.  Per array of hLambda, hMu, hDen:
    live cells             |got - ref| <= 1e-4 ref + 3 |alt - ref|      per cell (1e-4: TOL of tests/test_gpu_pseudo_hessian.py, whose docstring
                           measured a float32 accumulation of the same terms at 3.8e-6; the two oracle builds differ by <= 3.9e-6 per live
                           cell on the default seeds and the directed cases -- a factor 25 over either; measured on the GPU:
                           <= 1.4e-5, profiles/r17_pseudo_hessian_fuzz.txt)
    interior, not live     finite, >= 0 and <= 2e-30 x the array's constant
    outside the interior   exactly 0
    the whole array        max-norm deviation <= 1e-4 max ref + 3 max |alt - ref|,  |got - ref| <= 1e-4 |ref| + 3 |alt - ref|
A draw compared on less than 25 % of the ring or of the interior FAILS (fuzz_sides.PH_CAP): it is no xfail and no skip, this test
reports none.  Further per draw: arming changes no bit of misfit, gradients and gStf; a second armed call gives the same bits (no
atomics); under batch = 0 with several shots the call on all shots equals the float64 sum of the per-shot calls to 1e-6 per live cell
(float32 sets summed in double).

The directed cases (pseudo_hessian_ref.EDGE_CASES) put the launch geometry on its edges with dz = 0.8 dx and a ring that is live in
every cell: xmax on 63, 64, 127, 128 (the last row segment holds 64, 1, 64, 1 interior columns), nPml = 2 (the stencils reach index
0), nPml = 64 (seg0 = 1) without and with bottom padding, and rows x segments that leave idle waves in the last block, once with three
shots in one sub-batch and once with a forward lane used twice.  They are misfit-only calls: the accumulation is a forward-pass matter."""
import ctypes

import numpy as np
import pytest
import torch

import fuzz_common as C
import fuzz_draws as D
import problems as P
import pseudo_hessian_ref as R
from fuzz_sides import PH_CAP, describe_pseudo_hessian, pseudo_hessian_side

pytestmark = pytest.mark.gpu
TOL = 1e-4            # tests/test_gpu_pseudo_hessian.py
ADD_TOL = 1e-6


def compare(tag, H, ref, alt, pb):
    """The per-cell and whole-array bounds of the module docstring; prints the worst deviations, then asserts."""
    inside, ring = R.masks(pb)
    misses, lines = [], []
    interior, on_ring = R.live_shares(ref, pb)
    for name, g, w, a, live, const in zip(R.NAMES, H, ref, alt, R.live_cells(ref, pb["para"]["dt"]), R.constants(pb["para"]["dt"])):
        assert g.shape == w.shape and np.isfinite(g).all(), (tag, name)
        g64, spread = g.astype(np.float64), np.abs(a - w)
        dev = np.abs(g64 - w)
        on, below = live & inside, inside & ~live
        cell = float((dev[on] / w[on]).max()) if on.any() else 0.0
        cell_ring = float((dev[on & ring] / w[on & ring]).max()) if (on & ring).any() else 0.0
        dmax, l2 = float(dev.max() / w.max()), P.rel_l2(g, w)
        lines.append("%s: per live cell %.2e (ring %.2e), max-norm %.2e of the maximum, rel-L2 %.2e" % (name, cell, cell_ring, dmax, l2))
        bad = on & (dev > TOL * w + C.YARD * spread)
        if bad.any():
            z, x = np.argwhere(bad)[0]
            misses.append("%s: %d live cells miss their bound, the first (z %d, x %d): got %.6e, reference %.6e, other build %.6e" % (name, int(bad.sum()), z, x, g[z, x], w[z, x], a[z, x]))
        if not ((g[below] >= 0).all() and (g[below] <= 2.0 * R.FLOOR * const).all()):
            misses.append("%s: an interior cell below the floor holds %.3e" % (name, float(np.abs(g[below]).max())))
        if not (g[~inside] == 0).all():
            misses.append("%s: %d cells outside the interior are not 0" % (name, int((g[~inside] != 0).sum())))
        if not (dev.max() <= TOL * w.max() + C.YARD * spread.max() and C.array_held(g, w, a, TOL)):
            misses.append("%s: the whole array misses its bound (max-norm %.2e, rel-L2 %.2e)" % (name, dmax, l2))
    print("pseudo-Hessian %s: %s" % (tag, "; ".join(lines)))
    assert interior >= PH_CAP and on_ring >= PH_CAP, (tag, "compared on %.2f of the interior and %.2f of the ring: not tested" % (interior, on_ring))
    assert not misses, (tag, misses)


def same_bits(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(x, y), (what, k, float(np.abs(x.astype(np.float64) - y).max()))


def call(hip_ops, pb, h, ids=None, armed=True):
    """One call of the entry point h["entry"] at lame_init, armed with h["every"] as h["fetch"] says or plain.
    -> (misfit [, gLambda, gMu, gDen, gStf] as numpy, [hLambda, hMu, hDen] numpy or None)"""
    from sepfwi import _native
    fn = pb["para_fname"]
    ids = pb["Shot_ids"] if ids is None else torch.as_tensor(ids, dtype=torch.int32)
    n = 1 if h["entry"] == "forward" else 5

    def run(**kw):
        if h["entry"] == "forward":
            out = hip_ops.forward(*pb["lame_init"], pb["Stf"], 0, ids, fn, **kw)
        else:
            out = hip_ops.backward(*pb["lame_init"], pb["Stf"], 1, ids, fn, **kw)
        return [t.cpu().numpy().copy() for t in out]

    if not armed:
        out = run()
        assert len(out) == n
        return out, None
    if h["fetch"] == "ops":
        out = run(pseudo_hessian=h["every"])
        assert len(out) == n + 3
        return out[:n], out[n:]
    L = _native.lib()      # through the C ABI into host memory: the operator call itself is the plain one
    _native.check(L.sepfwi_pseudo_hessian_arm(fn.encode(), 0, h["every"]))
    try:
        out = run()
        H = [np.full((pb["nz_pad"], pb["nx_pad"]), -1.0, np.float32) for _ in range(3)]
        _native.check(L.sepfwi_get_pseudo_hessian(fn.encode(), 0, *[ctypes.c_void_p(a.ctypes.data) for a in H]))
    finally:
        L.sepfwi_pseudo_hessian_arm(fn.encode(), 0, 0)
    assert len(out) == n
    return out, H


@pytest.mark.parametrize("seed", C.seeds("SEPFWI_PH_FUZZ"))
def test_random_problem_matches_definition_cell_by_cell(tmp_path, oracle, oracle_nvfma, hip_ops, seed):
    from sepfwi import fwi_ops
    o, scale = C.settle(pseudo_hessian_side, tmp_path, oracle, oracle_nvfma, seed)
    assert o is not None, seed
    d, h = o["d"], o["h"]
    pb, opts = d["pb"], h["opts"]
    tag = "fuzz seed %d (%s)" % (seed, describe_pseudo_hessian(o, scale))
    ids = pb["Shot_ids"].tolist()
    fwi_ops.release()
    with P.kernel_options(**opts):
        hip_ops.obscalc(*D.observed_model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
        plain, _ = call(hip_ops, pb, h, armed=False)
        out, H = call(hip_ops, pb, h)
        _, again = call(hip_ops, pb, h)
        parts = [call(hip_ops, pb, h, ids=[sid])[1] for sid in ids] if opts.get("batch") == 0 and len(ids) > 1 else None
    fwi_ops.release()
    compare(tag, H, o["ref"], o["alt"], pb)
    same_bits(out, plain, (tag, "armed against disarmed: misfit, gradients, gStf"))
    assert np.isfinite(out[0]).all() and float(out[0].reshape(-1)[0]) > 0, tag
    same_bits(again, H, (tag, "a second armed call"))
    if parts is not None:
        inside, _ = R.masks(pb)
        worst = 0.0
        for name, g, live, k in zip(R.NAMES, H, R.live_cells(o["ref"], pb["para"]["dt"]), range(3)):
            total = sum(p[k].astype(np.float64) for p in parts)
            on = live & inside
            assert all(p[k].max() > 0 for p in parts), (tag, name)
            worst = max(worst, float((np.abs(g[on] - total[on]) / total[on]).max()))
        print("pseudo-Hessian %s: all %d shots against the float64 sum of the per-shot calls, per live cell %.2e" % (tag, len(ids), worst))
        assert worst <= ADD_TOL, (tag, worst)


@pytest.fixture(scope="module")
def edge_refs(oracle, oracle_nvfma, tmp_path_factory):
    """{case: (problem, options, reference, the other build's)} of the directed cases, the references computed once"""
    out = {}
    for name in R.EDGE_CASES:
        pb, opts = R.edge_problem(tmp_path_factory.mktemp("ph_edge"), name)
        args = [t.numpy() for t in pb["lame_init"]] + [pb["Stf"].numpy(), pb["Shot_ids"].numpy(), pb["para"], pb["survey"]]
        out[name] = (pb, opts, R.pseudo_hessian(oracle, *args)[0][1], R.pseudo_hessian(oracle_nvfma, *args)[0][1])
    return out


@pytest.mark.parametrize("name", list(R.EDGE_CASES))
def test_edges_of_the_launch_geometry_cell_by_cell(hip_ops, edge_refs, name):
    from sepfwi import fwi_ops
    pb, opts, ref, alt = edge_refs[name]
    g = R.EDGE_CASES[name][0]
    assert pb["para"]["dz"] == 0.8 * pb["para"]["dx"] and pb["nPml"] == g["nPml"] and pb["nPad"] == g["nPad"]
    assert R.live_shares(ref, pb) == (1.0, 1.0), (name, R.live_shares(ref, pb))      # every cell of the ring (and of the interior) is compared
    h = dict(entry="forward", fetch="ops", every=1)
    fwi_ops.release()
    with P.kernel_options(**opts):
        hip_ops.obscalc(*pb["lame_true"], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], to_store=True)
        plain, _ = call(hip_ops, pb, h, armed=False)
        out, H = call(hip_ops, pb, h)
    fwi_ops.release()
    compare("edge case %s (%d x %d nPml %d nPad %d, %d steps, %d shots, opts %r)" % (name, pb["nz_pad"], pb["nx_pad"], pb["nPml"], pb["nPad"], pb["nSteps"],
                                                                                  int(pb["Shot_ids"].numel()), opts), H, ref, alt, pb)
    same_bits(out, plain, (name, "armed against disarmed misfit"))
