"""The reference for the source block of Born modelling and of the exact adjoint (csrc/born.hpp, csrc/exact_adjoint.hpp "Source block";
sepfwi_born_src, sepfwi_adjoint_exact_src): nothing is restated.  The wavefield is exactly linear in the source time function, so
    J_s ds          js_ref: the CPU oracle's own forward gathers (oracle.cufd, calc_id 2) with stf = ds
and the adjoint side is DEFINED by it, as tests/exact_adjoint_ref.py defines J_m^T by born_ref:
    <J_s ds, w>     what <ds, g_stf> must equal (float64 on the host)
tests/test_stf_reference.py licenses js_ref on the CPU (oracle(stf + ds) - oracle(stf) = oracle(ds) to the two-build yardstick) and
shows that the end taper of the source rows is a pointwise window.  Either oracle build serves; the difference of the same quantity
between the two builds is the suite's yardstick for float32 rounding (tests/fuzz_common.py).

Layouts.  ds has the shape of Stf, (nSrc, nSteps): the oracle, like the library's Python surface, reads row shot_id.  The C ABI takes the
local layout, row i = shot_ids[i] (local_rows).

source_oracle_side is the oracle side of tests/test_gpu_source_adjoint_fuzz.py: fuzz_sides.exact_oracle_side (J_m v, J_m d, w = W J_m d of
born_ref on both builds) plus two seeded source perturbations and J_s of each, and the reference values of the identities, with no GPU."""
import numpy as np

import gauge_ref as GA
from born_ref import COMPS, ROW
from fuzz_common import has_target
from fuzz_sides import exact_oracle_side, oracle_gathers, wdot

DS_SEED0 = 7700
DS_SCALE = 0.02      # of max |stf|: J_s ds is then of the size of J_m v for the suite's v (1 % of the model), so that neither block drowns


def draw_ds(seed, stf, scale=1.0):
    """A seeded perturbation in the shape of stf (nSrc, nSteps), float32: white noise plus a smooth part of three times its size, about
    `scale` of max |stf|, every row different, first and last samples of every row at least half the amplitude -- a wrong taper or a wrong
    handling of column nSteps-1 shows."""
    stf = np.asarray(stf, np.float32)
    rng = np.random.default_rng(DS_SEED0 + seed)
    n, nt = stf.shape
    white = rng.uniform(-1.0, 1.0, (n, nt))
    k = np.hanning(max(5, nt // 12))
    smooth = np.stack([np.convolve(rng.uniform(-1.0, 1.0, nt + k.size - 1), k / k.sum(), mode="valid") for _ in range(n)])
    ds = 0.25 * white + 0.75 * smooth / max(np.abs(smooth).max(), 1e-300)
    for col in (0, nt - 1):
        s = np.where(ds[:, col] < 0, -1.0, 1.0)
        ds[:, col] = s * np.maximum(np.abs(ds[:, col]), 0.5)
    return np.ascontiguousarray(ds * scale * float(np.abs(stf).max()), dtype=np.float32)


def spike(stf, it, amp=None):
    """A unit spike (amp: max |stf|) at sample `it` of every row"""
    out = np.zeros_like(np.asarray(stf, np.float32))
    out[:, it] = float(np.abs(stf).max()) if amp is None else amp
    return out


def local_rows(ds, ids):
    """(nSrc, nSteps) -> the C ABI's (len(ids), nSteps): row i belongs to ids[i]"""
    return np.ascontiguousarray(np.asarray(ds, np.float32)[np.asarray(ids, np.int64)])


def gauge_cells(para):
    """G of the parameter key das_gauge_length, in cells along the fibre's axis (0: no gauge)"""
    dh = para["dz"] if para.get("das_fiber", "horizontal") == "vertical" else para["dx"]
    G = int(round(float(para.get("das_gauge_length", 0.0)) / float(dh)))
    return G if G > 1 else 0


def js_ref(oracle, model, ds, ids, para, survey):
    """J_s ds: the oracle's gathers at `model` with stf = ds -> per shot of ids {component: (nrec_i, nSteps) float64}.  With a gauge length
    the strain is the weighted mean of the member channels' and vx / vz are the centre member's, as tests/born_ref.born_side has them."""
    m = [np.ascontiguousarray(np.asarray(a), dtype=np.float32) for a in model]
    ds = np.ascontiguousarray(ds, dtype=np.float32)
    G = gauge_cells(para)
    if G:
        gauge, own = GA.forward(oracle, m, ds, ids, para, survey, G)
        return [dict(ett=np.asarray(g, np.float64), vx=o[1].astype(np.float64), vz=o[2].astype(np.float64)) for g, o in zip(gauge, own)]
    return [{c: a[ROW[c]] for c in COMPS} for a in oracle_gathers(oracle, m, ds, np.asarray(ids), para, survey)]


def plus(a, b):
    """per shot and component a + b (float64)"""
    return [{c: np.asarray(x[c], np.float64) + np.asarray(y[c], np.float64) for c in COMPS} for x, y in zip(a, b)]


def stf_dot(a, b, rows=None):
    """<a, b> of two (n, nSteps) arrays in float64; rows: those rows alone"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if rows is not None:
        a, b = a[rows], b[rows]
    return float((a * b).sum())


# ---- the two entry points straight through the C ABI (torch and the library are imported where they are used) --------------------------
def _ptr(a):
    import ctypes as C
    return None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _where(arrs, host):
    """numpy arrays as float32 host memory or as HIP tensors; None stays None"""
    import torch
    if arrs is None:
        return None
    arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in arrs]
    return arrs if host else [torch.from_numpy(a).cuda() for a in arrs]


def _counts(pb, ids):
    return [len(pb["survey"]["shot%d" % int(i)]["z_rec"]) for i in ids]


def born_src(pb, fn, v=None, ds=None, host=False, src_entry=True, ids=None, model="lame_init"):
    """ONE sepfwi_born_src call (sepfwi_born with src_entry=False).  v: three (nz, nx) arrays or None; ds: Stf's shape or None; host:
    every array in host memory.  -> per shot of ids {component: (nrec_i, nSteps) float32}"""
    import torch
    from sepfwi import _native
    L = _native.lib()
    ids = np.ascontiguousarray(pb["Shot_ids"].numpy() if ids is None else ids, dtype=np.int32)
    counts, nS = _counts(pb, ids), pb["nSteps"]
    n = max(1, sum(counts) * nS)
    outs = [np.zeros(n, np.float32) if host else torch.zeros(n, dtype=torch.float32, device="cuda") for _ in COMPS]      # ett, vx, vz
    m, vv = _where([t.numpy() for t in pb[model]], host), _where(v, host) or [None] * 3
    dl = None if ds is None else _where([local_rows(ds, ids)], host)[0]
    stf = np.ascontiguousarray(pb["Stf"].numpy(), dtype=np.float32)
    args = [_ptr(a) for a in outs] + [None] * 3 + [_ptr(a) for a in m + vv] + [_ptr(stf), 0, int(ids.size), _ptr(ids), fn.encode(), None]
    torch.cuda.synchronize()
    rc = L.sepfwi_born_src(*args, _ptr(dl)) if src_entry else L.sepfwi_born(*args)
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.sepfwi_last_error())
    off = np.concatenate([[0], np.cumsum(counts)]) * nS
    return [{c: _np(a)[off[i]:off[i + 1]].reshape(counts[i], nS) for c, a in zip(COMPS, outs)} for i in range(len(counts))]


def exact_src(pb, fn, v=None, w=None, ds=None, gstf=True, host=False, src_entry=True, ids=None, model="lame_init"):
    """ONE sepfwi_adjoint_exact_src call (sepfwi_adjoint_exact with src_entry=False).  w: {component: the gathers of the call's shots, shot
    after shot, any shape}.  -> ([gLambda, gMu, gDen], g_stf in the local layout (len(ids), nSteps) or None, misfit).  g_stf starts
    filled with 7: the call must overwrite every element."""
    import torch
    from sepfwi import _native
    L = _native.lib()
    ids = np.ascontiguousarray(pb["Shot_ids"].numpy() if ids is None else ids, dtype=np.int32)
    shape, nS = (pb["nz_pad"], pb["nx_pad"]), pb["nSteps"]
    g = [np.zeros(shape, np.float32) if host else torch.zeros(shape, dtype=torch.float32, device="cuda") for _ in range(3)]
    gs = None
    if gstf:
        gs = np.full((int(ids.size), nS), 7.0, np.float32) if host else torch.full((int(ids.size), nS), 7.0, dtype=torch.float32, device="cuda")
    m, vv = _where([t.numpy() for t in pb[model]], host), _where(v, host) or [None] * 3
    ww = [None] * 3
    if w is not None:
        ww = [None if c not in w else _where([np.asarray(w[c]).reshape(-1)], host)[0] for c in COMPS]
    dl = None if ds is None else _where([local_rows(ds, ids)], host)[0]
    stf = np.ascontiguousarray(pb["Stf"].numpy(), dtype=np.float32)
    misfit = np.zeros(1, np.float32)
    args = [_ptr(misfit)] + [_ptr(a) for a in g + ww + vv + m] + [_ptr(stf), 0, int(ids.size), _ptr(ids), fn.encode(), None]
    torch.cuda.synchronize()
    rc = L.sepfwi_adjoint_exact_src(*args, _ptr(dl), _ptr(gs)) if src_entry else L.sepfwi_adjoint_exact(*args)
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.sepfwi_last_error())
    return [_np(a) for a in g], (None if gs is None else _np(gs)), float(misfit[0])


# ---- the oracle side of the source fuzz ---------------------------------------------------------------------------------------------
def _source_side(lib, o, side, ds1, ds2):
    pb, sv = o["d"]["pb"], o["d"]["sv"]
    ids, weights = pb["Shot_ids"].numpy(), o["b"]["weights"] or (1.0, 0.0, 0.0)
    unit = (1.0, 1.0, 1.0)
    js1, js2 = (js_ref(lib, o["m"], ds, ids, pb["para"], sv) for ds in (ds1, ds2))
    u1, u2 = plus(side["jv"], js1), plus(side["jd"], js2)
    n = len(js1)
    return dict(js1=js1, js2=js2,
                sw=[wdot(js1, side["w"], unit, [i]) for i in range(n)],                 # <J_s ds1, w> per shot, w = W J_m d
                ns=[wdot(js1, js1, weights, [i]) for i in range(n)],                   # |W^1/2 J_s ds1|^2 per shot
                joint=wdot(u1, side["w"], unit),                                        # <J_m v + J_s ds1, w>
                n_u1=wdot(u1, u1, weights), n_s1=wdot(js1, js1, weights), n_u2=wdot(u2, u2, weights), cross=wdot(u1, u2, weights))


def source_oracle_side(tmp_path, oracle, oracle_nvfma, seed, scale):
    """exact_oracle_side's dict (None when the record is not live) with ["src"]: ds1, ds2 (Stf's shape), the reference values of both
    builds (ref, alt) and cmp = {comparison: (reference, the other build's, scale)}; ["target"] also asks every new yardstick to stay
    below 1e-2 of its scale."""
    o = exact_oracle_side(tmp_path, oracle, oracle_nvfma, seed, scale)
    if o is None:
        return None
    stf = o["d"]["pb"]["Stf"].numpy()
    ds1, ds2 = draw_ds(2 * seed, stf, DS_SCALE), draw_ds(2 * seed + 1, stf, DS_SCALE)
    r, a = _source_side(oracle, o, o["ref"], ds1, ds2), _source_side(oracle_nvfma, o, o["alt"], ds1, ds2)
    nd = o["ref"]["nd"]
    cmp = {"uHu [v;ds]": (r["n_u1"], a["n_u1"], abs(r["n_u1"])), "uHu [0;ds]": (r["n_s1"], a["n_s1"], abs(r["n_s1"])),
           "<u1,Hu2>": (r["cross"], a["cross"], float(np.sqrt(r["n_u1"] * r["n_u2"]))),
           "<[v;ds],JTw>": (r["joint"], a["joint"], float(np.sqrt(r["n_u1"] * nd)))}
    cmp["<ds,gstf>"] = (sum(r["sw"]), sum(a["sw"]), float(np.sqrt(r["n_s1"] * nd)))
    one = o["one"]      # per shot: the shot whose own record is live (exact_oracle_side), on its own scale
    cmp["<ds,gstf> shot %d" % one] = (r["sw"][one], a["sw"][one], float(np.sqrt(r["ns"][one] * o["ref"]["nd_one"])))
    yard = {k: abs(y - x) / max(s, 1e-300) for k, (x, y, s) in cmp.items()}
    o = dict(o)
    o["src"] = dict(ds1=ds1, ds2=ds2, ref=r, alt=a, cmp=cmp, yard=yard)
    o["target"] = o["target"] and all(s > 0 for _, _, s in cmp.values()) and has_target(*yard.values())
    return o
