"""Seeded random small problems for Born modelling J v and the Gauss-Newton product J^T W J v: HIP (csrc/born.hip,
csrc/session_born.cpp) vs the CPU oracle (-m gpu).

Every seed is a draw of tests/test_gpu_fuzz.py (fuzz_draws.draw_problem: grid, layer width, bottom padding, dz != dx, time step, frequency,
source depth, shots, receiver geometry, directional channels, water layer), changed from a generator of its own (fuzz_draws.draw_born,
default_rng(91000 + seed), so that the geometry of a seed stays what the other fuzz files see):
  * the conditioning keys leave the parameter file (the product is not defined with them); in one draw of four a SECOND parameter file
    keeps if_cross_misfit: with it gauss_newton must raise SepFwiError -1 and the Born gathers must equal the unconditioned ones bit for bit
  * the kernel options are one of BORN_OPTION_SETS: the structures born_tiled honours (bz, xcd_remap, rho_fly, amu_fly, rk_lazy), the
    two-launch backward step, quiet_skip = 1, no batching
  * in half of the multi-shot draws every shot has its own channel count, one shot a single channel
  * in one draw of four a joint misfit with weights (1, w_vx, w_vz), w in U(0.1, 1); in another one of four a gauge length G in 2 ... 5
    on a horizontal or vertical line of channels (reference: the member survey, tests/gauge_ref.py)

References (fuzz_sides.born_oracle_side, no GPU): the scattered gathers of tests/born_ref.py on BOTH oracle builds, and for the product
the oracle's gradient at the observed data obs_c = syn_c - (J v)_c formed from born_ref on the CPU (born_ref.shifted_gradient).  Yardsticks
and tolerances are those of tests/test_gpu_fuzz.py (tests/fuzz_common.py), none new:
    gathers   |got - ref| <= 1e-4 |ref| + 3 |alt - ref|                         per shot and component
    product   |hv - g|    <= (1e-3 + cond_g) |g| + 3 |g_alt - g|                per parameter, and below a water layer on its own
(obs = fl(syn - J v) carries half an ulp of syn into a residual of the size of J v: cond_g).
v^T H v / |W^1/2 J v|^2 is printed, for the GPU and for the oracle, and NOT asserted: the reference's adjoint is not the exact transpose
(0.23 ... 1.31 on the default seeds, the GPU and the oracle agreeing to four digits)."""
import ctypes

import numpy as np
import pytest
import torch

import fuzz_common as C
import problems as P
from born_ref import COMPS, GRADS
from fuzz_common import d64, l2, rel
from fuzz_sides import born_oracle_side, describe_born

pytestmark = pytest.mark.gpu


# ---- the GPU side ------------------------------------------------------------------------------------------------------------
def gpu_calls(hip_ops, pb, m, v, fn):
    """born and gauss_newton on device tensors -> (per shot {component: numpy}, [hvLambda, hvMu, hvDen] numpy)"""
    got = hip_ops.born(*m, *v, pb["Stf"], 1, pb["Shot_ids"], fn, components=COMPS)
    hv = hip_ops.gauss_newton(*m, *v, pb["Stf"], 1, pb["Shot_ids"], fn)
    return [{c: g[c].cpu().numpy() for c in COMPS} for g in got], [h.cpu().numpy() for h in hv]


def same_bits(a, b, what):
    (ga, ha), (gb, hb) = a, b
    assert len(ga) == len(gb), what
    for i, (x, y) in enumerate(zip(ga, gb)):
        for c in COMPS:
            assert x[c].shape == y[c].shape and np.array_equal(x[c], y[c]), (what, "shot %d" % i, c)
    for k, (x, y) in enumerate(zip(ha, hb)):
        assert np.array_equal(x, y), (what, "hv" + GRADS[k][1:])


def capi_born(pb, fn, counts, model, v, host_out):
    """ONE sepfwi_born call (gathers and product together) straight through the C ABI.  model / v: three arrays each, numpy (host
    memory) or HIP tensors; outputs in host memory (numpy) when host_out, else HIP tensors.  -> as gpu_calls."""
    from sepfwi import _native
    L = _native.lib()
    nS = int(pb["para"]["nSteps"])
    total = int(sum(counts)) * nS
    shape = (pb["nz_pad"], pb["nx_pad"])
    if host_out:
        outs, hvs = [np.zeros(total, np.float32) for _ in range(3)], [np.zeros(shape, np.float32) for _ in range(3)]
    else:
        outs = [torch.zeros(total, dtype=torch.float32, device="cuda") for _ in range(3)]
        hvs = [torch.zeros(shape, dtype=torch.float32, device="cuda") for _ in range(3)]
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    stf = np.ascontiguousarray(pb["Stf"].numpy(), dtype=np.float32)
    ids = np.ascontiguousarray(pb["Shot_ids"].numpy(), dtype=np.int32)
    torch.cuda.synchronize()
    rc = L.sepfwi_born(*[ptr(a) for a in outs + hvs + list(model) + list(v)], ptr(stf), 0, int(ids.size), ctypes.c_void_p(ids.ctypes.data), fn.encode(), None)
    _native.check(rc)
    torch.cuda.synchronize()
    host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
    ett, vx, vz = [host(a) for a in outs]
    got, off = [], 0
    for n in counts:
        got.append({c: a[off:off + n * nS].reshape(n, nS) for c, a in (("ett", ett), ("vx", vx), ("vz", vz))})
        off += n * nS
    return got, [host(a) for a in hvs]


@pytest.mark.parametrize("seed", C.seeds("SEPFWI_BORN_FUZZ"))
def test_random_problem_matches_oracle_born(tmp_path, oracle, oracle_nvfma, hip_ops, seed):
    """As test_random_problem_matches_oracle, with its re-draw of a record that ends before the wave reaches the channels."""
    from sepfwi import _native, fwi_ops
    o, scale = C.settled(born_oracle_side, tmp_path, oracle, oracle_nvfma, seed)
    d, b, ref, alt = o["d"], o["b"], o["ref"], o["alt"]
    pb, opts, w = d["pb"], b["opts"], d["water"]
    fn = pb["para_fname"]
    tag = (seed, describe_born(o, scale))
    quiet_total = None
    m_np, v_np = [np.ascontiguousarray(a, dtype=np.float32) for a in o["m"]], [np.ascontiguousarray(a, dtype=np.float32) for a in o["v"]]
    fwi_ops.release()
    with P.kernel_options(**opts):
        m = [torch.from_numpy(a).cuda() for a in m_np]
        v = [torch.from_numpy(a).cuda() for a in v_np]
        if opts.get("quiet_skip"):
            # a plain misfit call with quiet_skip = 1 first: it leaves quiet maps behind in the session that then serves the Born calls
            hip_ops.obscalc(*[t.cuda() for t in pb["lame_true"]], pb["Stf"], 1, pb["Shot_ids"], fn)
            hip_ops.forward(*m, pb["Stf"], 0, pb["Shot_ids"], fn)
            # (> 0 only where the channels are a fused line: a gauge or a joint misfit keeps the option off, and the line then reports 0;
            # tests/test_gpu_born.py holds the case with live maps on a fixed problem)
            quiet_total = hip_ops.stats(fn)["quiet_total"]
        first = gpu_calls(hip_ops, pb, m, v, fn)
        # 3. the same calls a second time in the same session: the same bits
        same_bits(first, gpu_calls(hip_ops, pb, m, v, fn), (tag, "second call of the session"))
        # 4. host memory through the C ABI: one call for gathers and product, bit-identical to the device-tensor calls
        same_bits(first, capi_born(pb, fn, b["counts"], m_np, v_np, False), (tag, "model and v in host memory"))
        same_bits(first, capi_born(pb, fn, b["counts"], m, v_np, False), (tag, "v in host memory, the model on the device"))
        same_bits(first, capi_born(pb, fn, b["counts"], m, v, True), (tag, "outputs in host memory"))
        if b["cond_fname"]:     # a live conditioning key: the product is refused, the gathers are the unconditioned ones
            with pytest.raises(_native.SepFwiError) as e:
                hip_ops.gauss_newton(*m, *v, pb["Stf"], 1, pb["Shot_ids"], b["cond_fname"])
            assert e.value.code == -1, (tag, str(e.value))
            cond = hip_ops.born(*m, *v, pb["Stf"], 1, pb["Shot_ids"], b["cond_fname"], components=COMPS)
            for i, g in enumerate(cond):
                for c in COMPS:
                    assert np.array_equal(g[c].cpu().numpy(), first[0][i][c]), (tag, "conditioned twin", i, c)
    if opts.get("quiet_skip"):      # ... and they equal those of a fresh session that never saw quiet_skip
        fwi_ops.release()
        with P.kernel_options(quiet_skip=0):
            same_bits(first, gpu_calls(hip_ops, pb, m, v, fn), (tag, "fresh session with quiet_skip = 0"))
    fwi_ops.release()
    got, hv = first
    assert len(got) == len(o["dsyn"]) == len(b["counts"]), (tag, len(got), len(o["dsyn"]))
    dev = {}
    # 1. the scattered gathers, per shot and component, on the two-build yardstick
    for i, (g, r, a) in enumerate(zip(got, o["dsyn"], o["dsyn_alt"])):
        for c in COMPS:
            assert g[c].shape == r[c].shape and np.isfinite(g[c]).all(), (tag, i, c, g[c].shape, r[c].shape)
            dev["d" + c] = max(dev.get("d" + c, (0.0, 0.0)), (rel(d64(g[c], r[c]), r[c]), rel(d64(a[c], r[c]), r[c])))
    print_line = lambda: print("born fuzz seed %d (%s): %r" % (seed, tag[1], {k: ("%.2e" % val[0], "%.2e" % val[1]) if isinstance(val, tuple) else "%.4g" % val for k, val in dev.items()}))
    for i, (g, r, a) in enumerate(zip(got, o["dsyn"], o["dsyn_alt"])):
        for c in COMPS:
            if not C.array_held(g[c], r[c], a[c], C.GATHER_TOL):
                print_line()
                raise AssertionError((tag, "shot %d" % i, c, rel(d64(g[c], r[c]), r[c]), rel(d64(a[c], r[c]), r[c])))
    # 2. the product against the oracle's gradient at obs = syn - J v
    cond_g = o["cond_g"]
    for k, name in enumerate(GRADS):
        dev["hv" + name[1:]] = (rel(d64(hv[k], ref[name]), ref[name]), rel(d64(alt[name], ref[name]), ref[name]))
    # 5. printed, not asserted
    dev["cond_g"] = cond_g
    if quiet_total is not None:
        dev["quiet_total of the priming call"] = quiet_total
    dev["vHv/|Jv|^2 GPU"] = sum(float((a.astype(np.float64) * h.astype(np.float64)).sum()) for a, h in zip(v_np, hv)) / ref["jv2"]
    dev["vHv/|Jv|^2 oracle"] = o["ratio"]
    print_line()
    if not o["target"]:
        pytest.xfail("seed %d: no parity target for the product -- the reference algorithm differs from itself by %.1e of the gradient on this "
                     "draw (conditioning term %.1e)" % (seed, o["noise_rel"], cond_g))
    for k, name in enumerate(GRADS):
        assert np.isfinite(hv[k]).all() and l2(ref[name]) > 0, (tag, name)
        miss = C.gradient_miss(hv[k], ref[name], alt[name], C.GRAD_TOL, cond_g, w)
        assert not miss, (tag, name, miss, dev["hv" + name[1:]], cond_g)
