"""The reference for the exact discrete adjoint (csrc/exact_adjoint.hpp, sepfwi_adjoint_exact): J itself, outside the GPU.

Nothing on the adjoint side is restated here.  J is tests/born_ref.py (the CPU oracle's own stencil kernels applied to the scattered
field, confirmed against finite differences of the oracle's gathers), and the adjoint is DEFINED by it:
    <J v, w>            dot_ref: what <v, J^T w> must equal
    (J^T w)_k           <J e_k, w> for single-cell perturbations e_k (probe_dots)
    exact gradient      <g, v> = <J v, -W r> with r = obs - syn the oracle's own residuals (oracle_residuals)
all accumulated in float64.  Either oracle build serves; the difference of the same quantity between the two builds (plain and nvfma)
is the suite's yardstick for float32 rounding (tests/fuzz_common.py), used 3 x next to the gradient tolerance 1e-3 (held).

Omega (mask_omega): rows nPml+1 ... nz-nPad-nPml-1, columns nPml+1 ... nx-nPml-1 of the padded grid -- the physical interior without
its first row and first column, where sepfwi_adjoint_exact reads v and writes g."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import born_ref as B
from born_ref import COMPS, ROW
from fuzz_common import GRAD_TOL as TOL, scalar_held      # TOL: the suite's gradient tolerance (README parity statement)

WEIGHTS = [(1.0, 0.0, 0.0), (1.0, 0.5, 0.25)]      # the misfits of the fixed-problem tests: axial strain alone, and joint
PROBE_CELLS = [(0, 11, 40), (0, 30, 11), (1, 35, 99), (0, 13, 17), (0, 39, 50), (0, 38, 60), (0, 25, 45), (0, 25, 46)]
# (shot, row, column) of the padded 50 x 90 grid: Omega's first row, first column, last column (seen from shot 1: the wave of shot 0 does
# not reach it within the record); diagonal to the source of shot 0 (12, 16); next to the fibre row (40); one deep; an adjacent pair


def mask_omega(pb):
    """bool (nz_pad, nx_pad)"""
    nz, nx, nPml, nPad = pb["nz_pad"], pb["nx_pad"], pb["nPml"], pb["nPad"]
    m = np.zeros((nz, nx), bool)
    m[nPml + 1:nz - nPad - nPml, nPml + 1:nx - nPml] = True
    return m


def on_omega(pb, v):
    m = mask_omega(pb)
    return [B.f32(np.where(m, a, 0.0)) for a in v]


def smooth_v(pb, seed, water_rows=0):
    """born_ref.perturbation masked to Omega (dMu zero in `water_rows` rows of water on top)"""
    return on_omega(pb, B.perturbation(pb, seed, water_rows=water_rows))


def white_v(pb, seed, water_rows=0):
    """white noise on Omega, every parameter, about 1 % of the model's size: a staggering error of one cell decorrelates it completely"""
    rng = np.random.default_rng(seed)
    v = [B.f32(rng.uniform(-1.0, 1.0, m.shape) * 0.01 * float(np.abs(m.numpy()).mean())) for m in pb["lame_init"]]
    v[1][:int(water_rows)] = 0.0
    return on_omega(pb, v)


def jv_ref(lib, pb, v, para=None, survey=None, ids=None, model="lame_init"):
    """born_ref J v -> {component: (nshots, nrec, nSteps) float32}"""
    ids = pb["Shot_ids"].numpy() if ids is None else np.asarray(ids)
    d = B.born(lib, *[t.numpy() for t in pb[model]], *v, pb["Stf"].numpy(), ids, para or pb["para"], survey or pb["survey"])["dsyn"]
    return {c: d[:, ROW[c]] for c in COMPS}


def data_dot(a, b, weights=(1.0, 0.0, 0.0)):
    """sum_c w_c <a_c, b_c> in float64; a, b: {component: array}.  Column 0 is 0 in every J v."""
    return sum(w * float((np.asarray(a[c], np.float64) * np.asarray(b[c], np.float64)).sum()) for c, w in zip(COMPS, weights) if w > 0)


def model_dot(a, b):
    return sum(float((np.asarray(x, np.float64) * np.asarray(y, np.float64)).sum()) for x, y in zip(a, b))


def cosine(a, b, weights):
    return data_dot(a, b, weights) / np.sqrt(data_dot(a, a, weights) * data_dot(b, b, weights))


def dot_ref(lib, pb, v, w, weights=(1.0, 0.0, 0.0), **kw):
    """<W J v, w>"""
    return data_dot(jv_ref(lib, pb, v, **kw), w, weights)


def unit_cell(pb, param, z, x, scale=1.0):
    v = [np.zeros((pb["nz_pad"], pb["nx_pad"]), np.float32) for _ in range(3)]
    v[param][z, x] = scale
    return v


def probe_dots(lib, pb, param, cells, w, weights=(1.0, 0.0, 0.0), scale=1.0, norms=False):
    """cells [(shot, z, x)], w {component: (nshots, nrec, nSteps)} -> float64 array of <J e_k, w> over the one shot named with the cell,
    e_k = `scale` in cell (z, x) of parameter `param` (the result is divided by scale): (J^T w)_k of that shot.  The runs are
    independent and ctypes drops the GIL: a few at a time.  norms=True: -> |J e_k| instead (w unused)."""
    def one(c):
        sid, z, x = c
        jv = jv_ref(lib, pb, unit_cell(pb, param, z, x, scale=scale), ids=[sid])
        if norms:
            return np.sqrt(data_dot(jv, jv, weights)) / scale
        return data_dot(jv, {k: a[sid:sid + 1] for k, a in w.items()}, weights) / scale
    with ThreadPoolExecutor(max_workers=8) as ex:
        return np.array(list(ex.map(one, cells)), np.float64)


def oracle_residuals(lib, pb, weights=(1.0, 0.0, 0.0)):
    """Observed data from lame_true, synthetics from lame_init, both the oracle's (calc_id 2 gathers).
    -> obs, r = obs - syn ({component: (nshots, nrec, nSteps)}, column 0 zero), misfit = 1/2 sum_c w_c |r_c|^2 over all columns."""
    stf, ids = pb["Stf"].numpy(), pb["Shot_ids"].numpy()
    g = lambda model: lib.cufd(*[t.numpy() for t in pb[model]], stf, 2, ids, pb["para"], pb["survey"])["syn"]
    o, s = g("lame_true"), g("lame_init")
    obs = {c: o[:, ROW[c]] for c in COMPS}
    r = {c: (o[:, ROW[c]].astype(np.float64) - s[:, ROW[c]].astype(np.float64)) for c in COMPS}
    return obs, r, 0.5 * data_dot(r, r, weights)


# ---- what the GPU tests of the pass share (torch and the library are imported where they are used: this module needs neither) -------
def held(got, ref, alt, what, scale=None):
    """|got - ref| <= 1e-3 scale + 3 |alt - ref|  (scale: |ref| unless given); prints the deviation first"""
    scale = abs(ref) if scale is None else scale
    dev, yard = abs(got - ref) / max(scale, 1e-300), abs(alt - ref) / max(scale, 1e-300)
    print("exact adjoint %s: got %.8e, reference %.8e, deviation %.2e of the scale (the two oracle builds %.2e)" % (what, got, ref, dev, yard))
    assert scalar_held(got, ref, alt, TOL, scale), (what, got, ref, dev, yard)


def outside_is_zero(pb, g, what):
    m = mask_omega(pb)
    for a in g:
        assert np.isfinite(a).all() and not np.any(a[~m]), what
    assert all(np.abs(a[m]).max() > 0 for a in g), what


def cuda(arrs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in arrs]


def capi(pb, fn, model, v=None, w=None, host_out=False):
    """ONE sepfwi_adjoint_exact call straight through the C ABI; model / v / w: numpy (host memory) or HIP tensors; the outputs in host
    memory when host_out.  -> (return code, [gLambda, gMu, gDen] numpy)"""
    import torch
    from sepfwi import _native
    L = _native.lib()
    shape = (pb["nz_pad"], pb["nx_pad"])
    g = [np.zeros(shape, np.float32) for _ in range(3)] if host_out else [torch.zeros(shape, dtype=torch.float32, device="cuda") for _ in range(3)]
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())
    stf = np.ascontiguousarray(pb["Stf"].numpy(), dtype=np.float32)
    ids = np.ascontiguousarray(pb["Shot_ids"].numpy(), dtype=np.int32)
    torch.cuda.synchronize()
    rc = L.sepfwi_adjoint_exact(None, *[ptr(a) for a in g], *[ptr(a) for a in (w or [None] * 3)], *[ptr(a) for a in (v or [None] * 3)],
                                *[ptr(a) for a in model], ptr(stf), 0, int(ids.size), C.c_void_p(ids.ctypes.data), fn.encode(), None)
    torch.cuda.synchronize()
    return rc, [a if isinstance(a, np.ndarray) else a.cpu().numpy() for a in g]
