"""The reference for the exact discrete adjoint (csrc/exact_adjoint.hpp, sepfwi_adjoint_exact): J itself, outside the GPU.

Nothing on the adjoint side is restated here.  J is tests/born_ref.py (the CPU oracle's own stencil kernels applied to the scattered
field, confirmed against finite differences of the oracle's gathers), and the adjoint is DEFINED by it:
    <J v, w>            dot_ref: what <v, J^T w> must equal
    (J^T w)_k           <J e_k, w> for single-cell perturbations e_k (probe_dots)
    exact gradient      <g, v> = <J v, -W r> with r = obs - syn the oracle's own residuals (oracle_residuals)
all accumulated in float64.  Either oracle build serves; the difference of the same quantity between the two builds (plain and nvfma)
is the suite's yardstick for float32 rounding (tests/test_gpu_born_fuzz.py), used 3 x next to the gradient tolerance 1e-3.

Omega (mask_omega): rows nPml+1 ... nz-nPad-nPml-1, columns nPml+1 ... nx-nPml-1 of the padded grid -- the physical interior without
its first row and first column, where sepfwi_adjoint_exact reads v and writes g."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import born_ref as B

COMPS = ("ett", "vx", "vz")
ROW = {"ett": 3, "vx": 1, "vz": 2}      # row of the component in born_ref's gathers [pr, vx, vz, ett]
TOL = 1e-3                              # the suite's gradient tolerance (README parity statement)


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
    return on_omega(pb, B.born_fuzz_perturbation(pb, seed, water_rows))


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
