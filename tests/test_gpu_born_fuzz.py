"""Seeded random small problems for Born modelling J v and the Gauss-Newton product J^T W J v: HIP (csrc/born.hip,
csrc/session_born.cpp) vs the CPU oracle (-m gpu).

Every seed is a draw of tests/test_gpu_fuzz.py (draw_problem: grid, layer width, bottom padding, dz != dx, time step, frequency, source
depth, shots, receiver geometry, directional channels, water layer), changed from a generator of its own (draw_born, default_rng(91000 +
seed), so that the geometry of a seed stays what the other fuzz files see):
  * the conditioning keys leave the parameter file (the product is not defined with them); in one draw of four a SECOND parameter file
    keeps if_cross_misfit: with it gauss_newton must raise SepFwiError -1 and the Born gathers must equal the unconditioned ones bit for bit
  * the kernel options are one of OPTION_SETS: the structures born_tiled honours (bz, xcd_remap, rho_fly, amu_fly, rk_lazy), the
    two-launch backward step, quiet_skip = 1, no batching
  * in half of the multi-shot draws every shot has its own channel count, one shot a single channel
  * in one draw of four a joint misfit with weights (1, w_vx, w_vz), w in U(0.1, 1); in another one of four a gauge length G in 2 ... 5
    on a horizontal or vertical line of channels (reference: the member survey, tests/gauge_ref.py)

References: the scattered gathers of tests/born_ref.py on BOTH oracle builds, and for the product the oracle's gradient at the observed
data obs_c = syn_c - (J v)_c formed from born_ref on the CPU (oracle.cufd, geophone_ref.cufd with weights, gauge_ref.reference) -- a
reference outside the GPU, where an error shared by sepfwi_born's two halves cannot cancel.  Yardsticks and tolerances are those of
tests/test_gpu_fuzz.py, none new:
    gathers   |got - ref| <= 1e-4 |ref| + 3 |alt - ref|                         per shot and component
    product   |hv - g|    <= (1e-3 + cond_g) |g| + 3 |g_alt - g|                per parameter, and below a water layer on its own
with cond_g = 4 eps sqrt(E / misfit) as defined there (obs = fl(syn - J v) carries half an ulp of syn into a residual of the size of J v).
v^T H v / |W^1/2 J v|^2 is printed, for the GPU and for the oracle, and NOT asserted: the reference's adjoint is not the exact transpose
(0.23 ... 1.31 on the default seeds, the GPU and the oracle agreeing to four digits).

The oracle side of a draw (oracle_side) needs no GPU: tests/test_born_fuzz_reference.py runs it on the default seeds, asserts that every
one has a live record and a parity target (so the xfail branch below is never what the default seeds report), confirms born_ref on each
draw against finite differences of the oracle's gathers, and holds a digest of what draw_born draws."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import born_ref as B
import gauge_ref as GA
import geophone_ref as GR
import problems as P
import test_gpu_fuzz as F

pytestmark = pytest.mark.gpu

BORN_SEED0 = 91000
OPTION_SETS = [dict(), dict(bz=1), dict(bz=4), dict(xcd_remap=0), dict(rho_fly=0), dict(amu_fly=0), dict(rk_lazy=0), dict(bwd_fuse=0),
               dict(quiet_skip=1), dict(batch=0)]
COMPS = ("ett", "vx", "vz")
ROW = {"ett": 3, "vx": 1, "vz": 2}      # row of the component in the reference's gathers [pr, vx, vz, ett]
GRADS = ("gLambda", "gMu", "gDen")

_SEEDS = ([int(v) for v in os.environ["SEPFWI_BORN_FUZZ_SEEDS"].split(",")] if os.environ.get("SEPFWI_BORN_FUZZ_SEEDS")
          else list(range(int(os.environ.get("SEPFWI_BORN_FUZZ_N", "16")))))


def _l2(a):
    return float(np.linalg.norm(np.asarray(a, np.float64)))


def _d64(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)))


def draw_born(d, seed):
    """Changes the draw d (test_gpu_fuzz.draw_problem) as the module docstring says and rewrites its two files.  Every quantity is drawn
    for every seed, used or not, so that one ingredient never shifts another.
    -> dict(opts, cond_fname (or None), ragged, counts, weights ((1, w_vx, w_vz) or None), G (0: none), vertical)."""
    pb, sv = d["pb"], d["sv"]
    nPml, nPad = pb["nPml"], pb["nPad"]
    nz, nx = pb["nz_pad"] - 2 * nPml - nPad, pb["nx_pad"] - 2 * nPml
    nshots = int(pb["Shot_ids"].numel())
    rg = np.random.default_rng(BORN_SEED0 + seed)
    want_cond = int(rg.integers(0, 4)) == 0
    opts = OPTION_SETS[int(rg.integers(0, len(OPTION_SETS)))]
    want_ragged = bool(rg.integers(0, 2))
    mode = int(rg.integers(0, 4))                     # 0: joint weights, 1: gauge length, 2 and 3: the draw's own channels and misfit
    w_vx, w_vz = [float(np.round(w, 3)) for w in rg.uniform(0.1, 1.0, 2)]
    G = int(rg.integers(2, 6))
    vertical = bool(rg.integers(0, 2))
    stride, start, cross_u = int(rg.integers(1, G + 2)), int(rg.integers(0, 3)), float(rg.uniform())
    para = {k: v for k, v in pb["para"].items() if k not in GA.COND_KEYS}
    if mode == 1:       # a line of gauge channels along the gauge's axis, every member inside the physical grid
        h = G // 2
        na, nc = (nz, nx) if vertical else (nx, nz)
        along = np.arange(h + 1 + start, na - h - 1, stride)
        cross = np.full(along.size, 2 + int(cross_u * (nc - 4)))
        z, x = (along, cross) if vertical else (cross, along)
        for k in range(nshots):
            sh = sv["shot%d" % k]
            sh["z_rec"], sh["x_rec"], sh["nrec"] = [int(a) for a in z], [int(a) for a in x], int(along.size)
            sh.pop("das_sensitivity", None)
        para.pop("das_fiber", None)
        if vertical:
            para["das_fiber"] = "vertical"
        para["das_gauge_length"] = G * float(para["dz"] if vertical else para["dx"])
    else:
        G, vertical = 0, para.get("das_fiber", "horizontal") == "vertical"
    weights = None
    if mode == 0:
        weights = (1.0, w_vx, w_vz)
        para.update(misfit_w_ett=1.0, misfit_w_vx=w_vx, misfit_w_vz=w_vz)
    n = int(sv["shot0"]["nrec"])
    counts = [int(c) for c in rg.integers(1, n + 1, size=nshots)]
    single = int(rg.integers(0, nshots))
    ragged = want_ragged and nshots > 1 and n > 1
    if ragged:
        counts[single] = 1
        if len(set(counts)) == 1:
            counts[(single + 1) % nshots] = n
        for k in range(nshots):
            sh = sv["shot%d" % k]
            sh["z_rec"], sh["x_rec"], sh["nrec"] = sh["z_rec"][:counts[k]], sh["x_rec"][:counts[k]], counts[k]
            if "das_sensitivity" in sh:
                sh["das_sensitivity"] = sh["das_sensitivity"][:counts[k]]
    else:
        counts = [n] * nshots
    json.dump(sv, open(pb["survey_fname"], "w"))
    json.dump(para, open(pb["para_fname"], "w"))
    pb["para"] = para
    cond_fname = None
    if want_cond:       # the same problem with a live conditioning key, a session of its own (plain misfit: a joint one refuses the key)
        cond_fname = os.path.join(os.path.dirname(pb["para_fname"]), "para_cond.json")
        cdir = os.path.join(os.path.dirname(pb["para_fname"]), "Cond_Data")
        os.makedirs(cdir, exist_ok=True)
        json.dump(dict({k: val for k, val in para.items() if not k.startswith("misfit_w_")}, if_cross_misfit=True, data_dir_name=cdir), open(cond_fname, "w"))
    return dict(opts=opts, cond_fname=cond_fname, ragged=ragged, counts=counts, weights=weights, G=G, vertical=vertical)


def born_side(lib, pb, sv, b, m, v):
    """born_ref on one oracle build -> per shot {component: (nrec, nSteps)} of the background (syn) and the scattered (dsyn) gathers;
    with a gauge length the strain is the weighted mean of the member channels' (float64) and vx / vz are the centre member's."""
    stf, ids = pb["Stf"].numpy(), pb["Shot_ids"].numpy()
    G = b["G"]
    if G:
        plain = {k: val for k, val in pb["para"].items() if k != "das_gauge_length"}
        r = B.born(lib, *m, *v, stf, ids, plain, GA.member_survey(sv, G, b["vertical"]), stack=False)
        pick = lambda a: dict(ett=GA.gauge_of(a[3][None], G)[0], vx=GA.centre_of(a[1][None], G)[0], vz=GA.centre_of(a[2][None], G)[0])
    else:
        r = B.born(lib, *m, *v, stf, ids, pb["para"], sv, stack=False)
        pick = lambda a: {c: a[ROW[c]] for c in COMPS}
    return [pick(a) for a in r["syn"]], [pick(a) for a in r["dsyn"]], r


def shifted_gradient(lib, pb, sv, b, m, syn, dsyn):
    """The oracle's gradient at obs_c = syn_c - (J v)_c (float32 data, as a file would hold them) on one build.
    -> dict(gLambda, gMu, gDen (float64 sums over the shot groups), misfit, E: 0.5 sum w_c |obs_c|^2, jv2: |W^1/2 J v|^2)."""
    stf, ids = pb["Stf"].numpy(), [int(i) for i in pb["Shot_ids"].tolist()]
    para, G, weights = pb["para"], b["G"], b["weights"]
    w = dict(zip(COMPS, weights or (1.0, 0.0, 0.0)))
    obs = [{c: (np.asarray(s[c], np.float64) - np.asarray(ds[c], np.float64)).astype(np.float32) for c in COMPS} for s, ds in zip(syn, dsyn)]
    E = 0.5 * sum(w[c] * _l2(o[c]) ** 2 for o in obs for c in COMPS if w[c] > 0)
    jv2 = sum(w[c] * _l2(ds[c][:, 1:]) ** 2 for ds in dsyn for c in COMPS if w[c] > 0)
    out = {k: 0.0 for k in GRADS}
    misfit = 0.0
    if G:
        r = GA.reference(lib, m, stf, np.asarray(ids, np.int32), para, sv, G, [o["ett"] for o in obs])
        out = {k: r[k].astype(np.float64) for k in GRADS}
        misfit = r["misfit"]
    else:
        for grp in GA._groups(ids, sv):
            pos = [ids.index(i) for i in grp]
            full = np.zeros((len(grp), 4) + obs[pos[0]]["ett"].shape, np.float32)
            for j, p in enumerate(pos):
                for c in COMPS:
                    full[j, ROW[c]] = obs[p][c]
            if weights:
                r = GR.cufd(lib, *m, stf, 1, grp, para, sv, obs=full, weights=weights)
            else:
                r = lib.cufd(*m, stf, 1, np.asarray(grp, np.int32), para, sv, obs=full)
            for k in GRADS:
                out[k] = out[k] + r[k].astype(np.float64)
            misfit += float(r["misfit"])
    out.update(misfit=misfit, E=E, jv2=jv2)
    return out


def oracle_side(tmp_path, oracle, oracle_nvfma, seed, scale):
    """The draw and everything the two oracle builds say about it (no GPU).  -> None when the record ends before the wave reaches the
    channels (the caller draws again with a longer record), else a dict; ["target"] is False where the product has no parity target."""
    d = F.draw_problem(tmp_path, seed, scale)
    b = draw_born(d, seed)
    pb, sv = d["pb"], d["sv"]
    m = [t.numpy() for t in pb["lame_init"]]
    v = B.born_fuzz_perturbation(pb, seed, d["water"])
    syn, dsyn, raw = born_side(oracle, pb, sv, b, m, v)
    src_scale = float(np.abs(pb["Stf"].numpy()).max()) * 1500.0 ** 2 * float(pb["para"]["dt"])
    peak = max(float(np.abs(s["ett"]).max()) for s in syn)
    if os.environ.get("SEPFWI_FUZZ_DIAG"):
        print("seed %d scale %d: %r; max |ett| / src_scale = %.3e, water %d" % (seed, scale, {k: val for k, val in b.items() if k != "cond_fname"}, peak / src_scale, d["water"]))
    if peak < 3e-10 * src_scale:      # only the stencil's numerical precursor (test_gpu_fuzz.py)
        return None
    syn_alt, dsyn_alt, _ = born_side(oracle_nvfma, pb, sv, b, m, v)
    ref = shifted_gradient(oracle, pb, sv, b, m, syn, dsyn)
    alt = shifted_gradient(oracle_nvfma, pb, sv, b, m, syn_alt, dsyn_alt)
    # conditioning of the draw and the cap of the yardstick: the comment at the assertions of test_gpu_fuzz.py
    cond_g = 4.0 * 2.0 ** -24 * float(np.sqrt(ref["E"] / max(abs(ref["misfit"]), 1e-300)))
    noise_rel = max(_l2(alt[k] - ref[k]) / max(_l2(ref[k]), 1e-300) for k in GRADS)
    vhv = sum(float((a.astype(np.float64) * ref[k]).sum()) for a, k in zip(v, GRADS))
    return dict(d=d, b=b, m=m, v=v, syn=syn, dsyn=dsyn, dsyn_alt=dsyn_alt, raw=raw, ref=ref, alt=alt, cond_g=cond_g, noise_rel=noise_rel,
                ratio=vhv / ref["jv2"], target=(noise_rel <= 1e-2 and cond_g <= 1e-2))


def describe(o, scale):
    b, d = o["b"], o["d"]
    pb = d["pb"]
    return ("%d x %d nPml %d nPad %d dz/dx %.2f nSteps %d, %s%s%s%s%s%s, opts %r, scale %d"
            % (pb["nz_pad"], pb["nx_pad"], pb["nPml"], pb["nPad"], pb["para"]["dz"] / pb["para"]["dx"], d["nSteps"], "counts %r" % (b["counts"],),
               ", ragged" if b["ragged"] else "", ", weights %r" % (b["weights"],) if b["weights"] else "",
               ", G %d %s" % (b["G"], "vertical" if b["vertical"] else "horizontal") if b["G"] else "", ", water %d" % d["water"] if d["water"] else "",
               ", conditioned twin" if b["cond_fname"] else "", b["opts"], scale))


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
    ptr = lambda a: C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    stf = np.ascontiguousarray(pb["Stf"].numpy(), dtype=np.float32)
    ids = np.ascontiguousarray(pb["Shot_ids"].numpy(), dtype=np.int32)
    torch.cuda.synchronize()
    rc = L.sepfwi_born(*[ptr(a) for a in outs + hvs + list(model) + list(v)], ptr(stf), 0, int(ids.size), C.c_void_p(ids.ctypes.data), fn.encode(), None)
    _native.check(rc)
    torch.cuda.synchronize()
    host = lambda a: a if isinstance(a, np.ndarray) else a.cpu().numpy()
    ett, vx, vz = [host(a) for a in outs]
    got, off = [], 0
    for n in counts:
        got.append({c: a[off:off + n * nS].reshape(n, nS) for c, a in (("ett", ett), ("vx", vx), ("vz", vz))})
        off += n * nS
    return got, [host(a) for a in hvs]


@pytest.mark.parametrize("seed", _SEEDS)   # one-off sweeps: SEPFWI_BORN_FUZZ_N=200 (CPU-oracle bound)
def test_random_problem_matches_oracle_born(tmp_path, oracle, oracle_nvfma, hip_ops, seed):
    """As test_random_problem_matches_oracle: a draw whose record ends before the wave reaches the channels is drawn again with the
    record two, then four times as long."""
    for scale in (1, 2, 4):
        if _attempt(tmp_path / ("x%d" % scale), oracle, oracle_nvfma, hip_ops, seed, scale):
            return
    pytest.xfail("seed %d: the wave does not reach the channels even with a record four times as long" % seed)


def _attempt(tmp_path, oracle, oracle_nvfma, hip_ops, seed, scale):
    from sepfwi import _native, fwi_ops
    o = oracle_side(tmp_path, oracle, oracle_nvfma, seed, scale)
    if o is None:
        return False
    d, b, ref, alt = o["d"], o["b"], o["ref"], o["alt"]
    pb, opts, w = d["pb"], b["opts"], d["water"]
    fn = pb["para_fname"]
    tag = (seed, describe(o, scale))
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
            err, noise = _d64(g[c], r[c]), _d64(a[c], r[c])
            dev["d" + c] = max(dev.get("d" + c, (0.0, 0.0)), (err / max(_l2(r[c]), 1e-300), noise / max(_l2(r[c]), 1e-300)))
    print_line = lambda: print("born fuzz seed %d (%s): %r" % (seed, tag[1], {k: ("%.2e" % val[0], "%.2e" % val[1]) if isinstance(val, tuple) else "%.4g" % val for k, val in dev.items()}))
    for i, (g, r, a) in enumerate(zip(got, o["dsyn"], o["dsyn_alt"])):
        for c in COMPS:
            if not _d64(g[c], r[c]) <= 1e-4 * _l2(r[c]) + 3.0 * _d64(a[c], r[c]):
                print_line()
                raise AssertionError((tag, "shot %d" % i, c, _d64(g[c], r[c]) / max(_l2(r[c]), 1e-300), _d64(a[c], r[c]) / max(_l2(r[c]), 1e-300)))
    # 2. the product against the oracle's gradient at obs = syn - J v
    cond_g = o["cond_g"]
    for k, name in enumerate(GRADS):
        dev["hv" + name[1:]] = (_d64(hv[k], ref[name]) / max(_l2(ref[name]), 1e-300), _l2(alt[name] - ref[name]) / max(_l2(ref[name]), 1e-300))
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
        r, a, g = ref[name], alt[name], hv[k]
        assert np.isfinite(g).all() and _l2(r) > 0, (tag, name)
        assert _d64(g, r) <= (1e-3 + cond_g) * _l2(r) + 3.0 * _l2(a - r), (tag, name, dev["hv" + name[1:]], cond_g)
        if w:   # below a water layer the image is held on its own (against the larger of its own norm and 3 % of the whole image's)
            yard = max(_l2(r[w:]), 3e-2 * _l2(r))
            assert _d64(g[w:], r[w:]) <= (1e-3 + cond_g) * yard + 3.0 * _l2(a[w:] - r[w:]), (tag, name, "below the water")
    return True
