"""Seeded random geometries for the persistent backward loop (-m gpu): grid size and aspect, layer width, bottom padding, record
length, shot positions, strip width and cost weights of the tiling, wave-priority scheme, LDS mask, imaging interval and the order of a tile's segments are drawn per case; the
loop must give the two-launch step's misfit, gradients and source gradients BIT FOR BIT (same bodies, same order of operations on
every array) -- which makes any stale halo read, any missed hand-off between tiles, visible.  No oracle involved: seconds per draw.
One-off sweeps: SEPFWI_PFUZZ_N=200 (profiles/r05_persist_fuzz.txt)."""
import os

import numpy as np
import pytest

import problems as P

pytestmark = pytest.mark.gpu

_SEEDS = list(range(int(os.environ.get("SEPFWI_PFUZZ_N", "6"))))


@pytest.mark.parametrize("seed", _SEEDS)
def test_persistent_loop_random_geometry_is_bit_identical(tmp_path, hip_ops, seed, probes_lib):
    rng = np.random.default_rng(4000 + seed)
    nPml = int(rng.integers(6, 33))
    # at least 4 x 512 row segments of 64 columns, i.e. every one of the 512 tiles gets a handful; aspect from 1 : 12 to 12 : 1
    while True:
        nz, nx = int(rng.integers(40, 900)), int(rng.integers(100, 2400))
        nPad = int(rng.integers(0, 9))
        segs = (nz + 2 * nPml) * ((nx + 2 * nPml + 63) // 64)
        if 2200 <= segs <= 14000:
            break
    nSteps = int(rng.integers(150, 420))
    nshots = int(rng.integers(1, 3))
    rec_z = int(rng.integers(2, max(3, min(nz - 3, 60))))
    pb = P.make_problem(str(tmp_path), nz=nz, nx=nx, nPml=nPml, nPad=nPad, nSteps=nSteps, nshots=nshots, hetero=True, seed=seed,
                        src_z=int(rng.integers(1, 5)), rec_z=rec_z, f0=float(rng.uniform(10.0, 30.0)))
    lt, mt, dt_ = pb["lame_true"]
    hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], to_store=True)
    lam, mu, den = pb["lame_init"]
    lam = (lam * 1.05).contiguous()
    common = dict(batch=0, img_every=int(rng.choice([1, 1, 1, 2, 3])), early=int(rng.choice([0, 0, 3])))
    loop = dict(pk_px=int(rng.integers(1, 9)), pk_lmask=int(rng.choice([16, 16, 31, 15, 7, 3, 1, 0])), pk_order=int(rng.integers(0, 2)),
                pk_wpc=int(rng.choice([2, 2, 2, 1])), pk_prio=int(rng.integers(0, 4)),
                # tiling by cost: weights of the absorbing strips from 0.7 to three times a plain segment (lighter strips would give their
                # tiles more segments than the explicit LDS masks drawn above can hold)
                pk_wx=int(rng.choice([150, 100, 70, 300])), pk_wxp=int(rng.choice([150, 100, 70, 250])), pk_wz=int(rng.choice([115, 100, 70, 220])))
    with P.kernel_options(bwd_fuse=2, **common):
        ref = [t.numpy().copy() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])]
    with P.kernel_options(bwd_fuse=4, **common, **loop):
        got = [t.numpy().copy() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])]
        steps = hip_ops.stats(pb["para_fname"], 0)["persist_steps"]
    hip_ops.release()      # (a sweep of thousands of draws would otherwise keep every draw's session and its arrays)
    desc = dict(seed=seed, nz=nz, nx=nx, nPml=nPml, nPad=nPad, nSteps=nSteps, nshots=nshots, **common, **loop)
    assert steps == nshots * (nSteps - 1), desc          # the loop really ran
    for name, a, b in zip(("misfit", "gLambda", "gMu", "gDen", "gStf"), got, ref):
        assert np.array_equal(a, b), (desc, name, float(np.abs(a - b).max()), float(np.abs(b).max()))
    assert np.isfinite(ref[0]).all() and np.abs(ref[4]).max() > 0, desc      # (the source gradient is alive from the first backward steps on)


_GSEEDS = list(range(int(os.environ.get("SEPFWI_GFUZZ_N", "6"))))


@pytest.mark.parametrize("seed", _GSEEDS)
def test_loop_general_receivers_random_geometry(tmp_path, hip_ops, seed):
    """Receivers that are not a fused line inside the persistent loop (folded adjoint source, k_bwd_persist<LMASK, GINJ>) against the
    two-launch step + k_inject on seeded random grids, layer widths and channel sets: strided, scattered with repeats and shared
    cells, a vertical fibre, directional sensitivities.  The two differ only in the order of the float adds into a cell that several
    channels reach (k_inject's atomics have none): gradients to 5e-6, misfit exactly.  Every odd seed draws a grid of 28 672 to 40 000
    row segments: from 56 segments per tile of an MI355X's 512 up, each tile walks its segments in strip order (session_persist.cpp's
    tile-size rule), as at the headline size; the even seeds' grids are smaller (edge-first order).  One-off sweeps: SEPFWI_GFUZZ_N=200."""
    rng = np.random.default_rng(9000 + seed)
    nPml = int(rng.integers(6, 25))
    big = seed % 2 == 1
    while True:
        if big:
            nz, nx = int(rng.integers(150, 1300)), int(rng.integers(600, 3000))
        else:
            nz, nx = int(rng.integers(60, 600)), int(rng.integers(120, 1800))
        segs = (nz + 2 * nPml) * ((nx + 2 * nPml + 63) // 64)
        if (28672 <= segs <= 40000) if big else (2200 <= segs <= 12000):
            break
    nSteps = int(rng.integers(150, 380))
    nshots = int(rng.integers(1, 3))
    kind = int(rng.integers(0, 4))
    kw = {}
    if kind == 0:
        kw = dict(nrec_stride=int(rng.integers(2, 7)), rec_z=int(rng.integers(2, max(3, min(nz - 3, 60)))))
    elif kind == 1:
        m = int(rng.integers(1, 60))
        xs = rng.integers(2, nx - 2, size=m)
        xs = np.concatenate([xs, xs[: m // 3], xs[: m // 4] + 1])      # repeated channels and neighbours that share a cell
        kw = dict(rec_x=[int(min(v, nx - 2)) for v in xs], rec_z=int(rng.integers(2, max(3, min(nz - 3, 60)))),
                  src_x=[int(np.clip(np.median(xs) + 25 * q, 2, nx - 3)) for q in range(nshots)])      # sources among the channels: the wave arrives within the record
    elif kind == 2:
        kw = dict(das_fiber="vertical", nrec_stride=int(rng.integers(1, 4)), src_x=[int(nx // 2 - 20), int(nx // 2 + 30)][:nshots])
    else:
        kw = dict(das_sensitivity="random", nrec_stride=int(rng.integers(1, 4)), rec_z=int(rng.integers(3, max(4, min(nz - 4, 60)))))
    pb = P.make_problem(str(tmp_path), nz=nz, nx=nx, nPml=nPml, nSteps=nSteps, nshots=nshots, hetero=True, seed=seed, f0=float(rng.uniform(10.0, 30.0)), **kw)
    lt, mt, dt_ = pb["lame_true"]
    hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], to_store=True)
    lam, mu, den = pb["lame_init"]
    lam = (lam * 1.05).contiguous()
    with P.kernel_options(batch=0, bwd_fuse=2):
        ref = [t.numpy().copy() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])]
    with P.kernel_options(batch=0, bwd_fuse=4):
        got = [t.numpy().copy() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])]
        steps = hip_ops.stats(pb["para_fname"], 0)["persist_steps"]
    hip_ops.release()
    import torch
    strip = segs >= 56 * 2 * torch.cuda.get_device_properties(0).multi_processor_count      # (the tile-size rule with 2 tiles per CU)
    desc = dict(seed=seed, nz=nz, nx=nx, nPml=nPml, nSteps=nSteps, nshots=nshots, kind=kind, nrec=pb["nrec"], segs=segs,
                order="strip" if strip else "edge-first")
    assert steps == nshots * (nSteps - 1), desc
    assert got[0][0] == ref[0][0], desc
    if not ref[0][0] > 0:      # (a record that ends before the wave reaches any channel: the "gradient" is rounding noise of the stencil's precursor)
        pytest.xfail("seed %d: no signal at the channels within the record" % seed)
    for name, a, b in zip(("gLambda", "gMu", "gDen", "gStf"), got[1:], ref[1:]):
        if np.abs(b).max() > 0:
            assert P.rel_l2(a, b) <= 5e-6, (desc, name, P.rel_l2(a, b))
        else:
            assert not a.any(), (desc, name)
