"""Who owns the memory (csrc/device_alloc.hpp): every device and pinned allocation of the library goes through one seam that counts
the live bytes of the process (test hook sepfwi_debug_live_bytes).  A refused session holds nothing, every session gives back all
it took, sepfwi_stats.device_bytes is what the session really holds, and growing the per-call tables changes no result.

Every test reads the live bytes as its baseline after fwi_ops.release() and asserts on differences from it, so nothing depends on
what else has run in the process (torch's own allocations do not go through the seam)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import problems as P
from conftest import ROOT
from sepfwi import _native

pytestmark = pytest.mark.gpu


def live():
    """(device bytes, pinned host bytes) the active build of the library holds right now"""
    d, p = C.c_longlong(-1), C.c_longlong(-1)
    _native.check(_native.lib().sepfwi_debug_live_bytes(C.byref(d), C.byref(p)))
    return d.value, p.value


def rewrite_para(pb, **keys):
    para = dict(pb["para"], **keys)
    with open(pb["para_fname"], "w") as fp:
        json.dump(para, fp)
    return para


# what a fresh process computes on the problem of test_a_refused_session_holds_nothing: the misfit's bits
_FRESH = """
import sys
sys.path[:0] = %r
import problems as P
from sepfwi import fwi_ops
pb = P.make_problem(sys.argv[1], nz=60, nx=80, nPml=10, nSteps=50, nshots=1, hetero=False)
fwi_ops.obscalc(*pb["lame_true"], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
lam, mu, den = pb["lame_init"]
print("MISFIT", fwi_ops.forward((lam * 1.05).contiguous(), mu, den, pb["Stf"], 0, pb["Shot_ids"], pb["para_fname"])[0].numpy().tobytes().hex())
"""


def test_a_refused_session_holds_nothing(tmp_path, hip_ops):
    """The "outside" case of test_gpu_das_gauge.py::test_gauge_errors_reach_the_c_abi: the survey check refuses the session AFTER its
    stream, events, arrays and tables exist.  Nothing of them is left (before the owning buffers the constructor's throw leaked all of
    it: profiles/r13_owned_buffers.txt has the figure), and the corrected file then builds a session whose misfit has the bits a
    fresh process computes."""
    hip_ops.release()
    base = live()
    pb = P.make_problem(str(tmp_path / "here"), nz=60, nx=80, nPml=10, nSteps=50, nshots=1, hetero=False)
    rewrite_para(pb, das_gauge_length=310.0)
    lt, mt, dt_ = pb["lame_true"]
    with pytest.raises(_native.SepFwiError) as e:
        hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    assert e.value.code == -1, str(e.value)
    after = live()
    print("live bytes after the refused session: device %+d, pinned %+d" % (after[0] - base[0], after[1] - base[1]))
    assert after == base
    rewrite_para(pb)
    hip_ops.obscalc(lt, mt, dt_, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    lam, mu, den = pb["lame_init"]
    got = hip_ops.forward((lam * 1.05).contiguous(), mu, den, pb["Stf"], 0, pb["Shot_ids"], pb["para_fname"])[0].numpy().tobytes().hex()
    assert live()[0] > base[0]
    out = subprocess.run([sys.executable, "-c", _FRESH % [p for p in sys.path if p.startswith(ROOT)], str(tmp_path / "fresh")],
                         capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stdout + out.stderr
    fresh = [ln.split()[1] for ln in out.stdout.splitlines() if ln.startswith("MISFIT")]
    assert fresh == [got] and np.isfinite(np.frombuffer(bytes.fromhex(got), np.float32)[0])
    hip_ops.release()
    assert live() == base


def test_every_session_gives_everything_back(tmp_path, hip_ops, probes_lib):
    """Sessions that together reach every block allocated, grown or replaced after the constructor: after each of them is released the
    live device and pinned bytes are back at the baseline."""
    hip_ops.release()
    base = live()
    seen = []

    def done(what, pb, **want):
        st = hip_ops.stats(pb["para_fname"], 0)
        for k, v in want.items():
            assert st[k] >= v, (what, k, st[k])
        now = live()
        assert now[0] - base[0] == st["device_bytes"] > 0, (what, now, base, st["device_bytes"])
        seen.append((what, now[0] - base[0], now[1] - base[1]))
        hip_ops.release()
        assert live() == base, (what, live(), base)

    def observe(pb, **kw):
        hip_ops.obscalc(*pb["lame_true"], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], to_store=True, **kw)

    def model(pb):
        lam, mu, den = pb["lame_init"]
        return (lam * 1.04).contiguous(), mu, den

    # the stream schedule with three forward lanes: without frames (a misfit call), then with them
    pb = P.make_problem(str(tmp_path / "lanes"), nshots=3)
    with P.kernel_options(batch=0, fwd_lanes=3):
        observe(pb)
        hip_ops.forward(*model(pb), pb["Stf"], 0, pb["Shot_ids"], pb["para_fname"])
        without = live()[0]
        hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
        assert live()[0] > without
        done("stream lanes", pb)

    # the batched schedule at the notebook's size: forward and backward arenas, then more shots -- arenas and tables are regrown
    pb = P.make_problem(str(tmp_path / "batched"), nz=101, nx=201, nPml=32, nSteps=380, nshots=7, hetero=True)
    with P.kernel_options(batch=1, bwd_fuse=2):
        observe(pb)
        hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"][:2], pb["para_fname"])
        few = live()[0]
        hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
        assert live()[0] > few
        done("batched", pb)

    # the persistent loop with receivers that are not a fused line (plan, tile_has, d_args, inj_val_), then another tiling
    pb = P.make_problem(str(tmp_path / "loop"), nz=300, nx=500, nPml=10, nSteps=420, nshots=2, hetero=True, rec_z=40, nrec_stride=3)
    with P.kernel_options(batch=0, bwd_fuse=4):
        observe(pb)
        hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
        assert hip_ops.stats(pb["para_fname"], 0)["persist_steps"] == 2 * (pb["nSteps"] - 1), hip_ops.loop_status(pb["para_fname"])
        one_tiling = live()
        with P.kernel_options(batch=0, bwd_fuse=4, pk_px=2):
            hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
            assert hip_ops.stats(pb["para_fname"], 0)["persist_steps"] == 2 * (pb["nSteps"] - 1), hip_ops.loop_status(pb["para_fname"])
            assert live()[1] == one_tiling[1] > base[1]      # (the pinned verdict words are kept across tilings)
            done("persistent loop, two tilings", pb)

    # a gauge length, in both schedules (taps, adjoint plan; the batched schedule's side table)
    pb = P.make_problem(str(tmp_path / "gauge"), nz=60, nx=80, nPml=10, nSteps=50, nshots=2, hetero=False)
    pb["para"] = rewrite_para(pb, das_gauge_length=3 * pb["para"]["dx"])
    observe(pb)
    for batch in (0, 1):
        with P.kernel_options(batch=batch):
            hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    done("gauge length", pb)

    # joint weights in the batched schedule (the residual table and the backward twin of the shot table)
    pb = P.make_problem(str(tmp_path / "joint"), nshots=3)
    pb["para"] = rewrite_para(pb, misfit_w_ett=1.0, misfit_w_vx=0.5, misfit_w_vz=2.0)
    with P.kernel_options(batch=1):
        observe(pb)
        hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
        done("joint weights", pb)

    # an armed pseudo-Hessian, Born modelling and the exact Gauss-Newton product
    pb = P.make_problem(str(tmp_path / "second_order"), nshots=2)
    observe(pb)
    assert len(hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], pseudo_hessian=2)) == 8
    v = [(0.01 * t).contiguous() for t in pb["lame_init"]]
    hip_ops.born(*model(pb), *v, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    hip_ops.gauss_newton(*model(pb), *v, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact=True)
    done("pseudo-Hessian, Born, exact product", pb)

    # a conditioning key with the source update (the conditioner's six blocks)
    pb = P.make_problem(str(tmp_path / "conditioned"), nshots=2)
    pb["para"] = rewrite_para(pb, filter=[3.0, 7.0, 40.0, 60.0], if_src_update=True)
    observe(pb)
    hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
    done("conditioning", pb)

    # a budget of the observed-data store small enough that gathers go to pinned host memory and come back
    pb = P.make_problem(str(tmp_path / "budget"), nz=40, nx=130, nPml=10, nSteps=1000, nshots=6, hetero=True)
    with P.kernel_options(batch=0, fwd_lanes=2, obs_cache_mb=1):
        observe(pb)
        hip_ops.backward(*model(pb), pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
        assert live()[1] - base[1] >= hip_ops.stats(pb["para_fname"], 0)["obs_host_bytes"] > 0
        done("observed-data budget", pb, obs_evictions=4, obs_host_bytes=1)

    for what, dev, pin in seen:
        print("%-40s held %12d device bytes, %9d pinned" % (what, dev, pin))
    hip_ops.release()
    assert live() == base


def test_device_bytes_is_what_the_session_holds(tmp_path, hip_ops, probes_lib):
    """sepfwi_stats.device_bytes of the one session alive equals the live device bytes above the baseline: after the first gradient
    call, a Born call, an armed call and a call with more shots.  Every block is counted at its real size while it is held -- and an
    allocation made outside the seam, or counted at another size, shows here."""
    hip_ops.release()
    base = live()
    pb = P.make_problem(str(tmp_path), nz=101, nx=201, nPml=32, nSteps=380, nshots=7, hetero=True)
    lam, mu, den = pb["lame_init"]
    m = ((lam * 1.04).contiguous(), mu, den)
    v = [(0.01 * t).contiguous() for t in pb["lame_init"]]
    fn, ids = pb["para_fname"], pb["Shot_ids"]
    hip_ops.obscalc(*pb["lame_true"], pb["Stf"], 1, ids, fn, to_store=True)
    steps = [("first gradient call", lambda: hip_ops.backward(*m, pb["Stf"], 1, ids[:2], fn)),
             ("Born call", lambda: hip_ops.born(*m, *v, pb["Stf"], 1, ids[:2], fn)),
             ("armed call", lambda: hip_ops.backward(*m, pb["Stf"], 1, ids[:2], fn, pseudo_hessian=3)),
             ("more shots", lambda: hip_ops.backward(*m, pb["Stf"], 1, ids, fn))]
    last = 0
    for what, call in steps:
        call()
        held, stat = live()[0] - base[0], hip_ops.stats(fn, 0)["device_bytes"]
        print("%-20s device_bytes %12d, live %12d" % (what, stat, held))
        assert stat == held, what
        assert held > last, what      # (each of the four takes blocks the ones before did not need)
        last = held
    hip_ops.release()
    assert live() == base


@pytest.mark.parametrize("batch", [1, 0], ids=["batched", "streams"])
def test_results_are_unchanged_across_a_regrow(tmp_path, hip_ops, batch):
    """2 shots, then 5, then 2 again in one session: the per-call tables and arenas are replaced by larger ones in the second call, and
    the third gives the first one's misfit and gradients bit for bit."""
    hip_ops.release()
    pb = P.make_problem(str(tmp_path), nshots=5)
    lam, mu, den = pb["lame_init"]
    lam = (lam * 1.04).contiguous()
    ids = pb["Shot_ids"]
    with P.kernel_options(batch=batch):
        hip_ops.obscalc(*pb["lame_true"], pb["Stf"], 1, ids, pb["para_fname"], to_store=True)
        runs = [[t.cpu().numpy().copy() for t in hip_ops.backward(lam, mu, den, pb["Stf"], 1, ids[:n], pb["para_fname"])] for n in (2, 5, 2)]
    assert runs[0][0][0] > 0 and runs[1][0][0] > runs[0][0][0]
    for name, a, b in zip(("misfit", "gLambda", "gMu", "gDen", "gStf"), runs[0], runs[2]):
        assert np.abs(a).max() > 0 and np.array_equal(a, b), name
    hip_ops.release()
