"""What the tests of the parameter chain's tangent share (tests/test_param_tangent_host.py, tests/test_gpu_param_tangent.py): seeded inputs
for the seven modules on a small grid, and the float64 references -- torch.func.jvp of the modules' own expression, its dense Jacobian.
Nothing of the code under test is restated: the references differentiate `lame(blend(padding(.)))` of a float64 copy of the module.

Bounds, none new: the project's own for the chain rule of these maps (tests/test_gpu_param_maps.py), per output array and relative to
that array's largest reference entry: 2e-6 for the five algebraic kinds, 1e-6 for the two rock-physics maps.

Inputs: a tangent of random sign can make the three terms of one output cancel at a cell (on a one-cell grid: everywhere), and the
deviation then measures the conditioning of that direction, not the code.  The seed below was chosen, before any GPU run, among 24 by
the float32 torch path and a host build of the kernel's per-cell arithmetic: largest deviation 1.9e-7 (algebraic kinds) and 5.9e-7 (rock
physics; dLambda = dk - 2/3 dmu loses a factor ~3.5 to cancellation for any input, so a third of 1e-6 is out of float32's reach)."""
import numpy as np
import torch

from sepfwi import modules as M
from sepfwi import utils as ft

CLASSES = ["FWI", "FWI_Lame_Den", "FWI_IP_IS_Den", "FWI_Vp_Vs_IP", "FWI_Vp_Vs_IS", "FWI_Rock_Physics_VRH", "FWI_Rock_Physics_gassmann"]
SEED = 21      # inputs() at this seed: the float32 evaluation of torch itself sits well inside the bounds on every grid of the tests
SMALL = (3, 5, 2, 1)       # (nz, nx, nPml, nPad): partial blocks in both directions


def tol_of(cls_name):
    return 1e-6 if "Rock" in cls_name else 2e-6


def fields(cls_name, rng, nz, nx):
    """three float64 (nz, nx) arrays in the module's own parameters"""
    if "Rock" in cls_name:
        return [rng.uniform(lo, hi, (nz, nx)) for lo, hi in ((0.10, 0.30), (0.05, 0.45), (0.2, 0.9))]
    vp = rng.uniform(2600.0, 3800.0, (nz, nx))
    vs = vp / rng.uniform(1.65, 1.85, (nz, nx))
    rho = rng.uniform(2100.0, 2600.0, (nz, nx))
    if cls_name == "FWI":
        return [vp, vs, rho]
    if cls_name == "FWI_Lame_Den":
        return [rho * (vp ** 2 - 2 * vs ** 2) / 1e6, rho * vs ** 2 / 1e6, rho]
    if cls_name == "FWI_IP_IS_Den":
        return [vp / 1e3 * rho, vs / 1e3 * rho, rho]
    if cls_name == "FWI_Vp_Vs_IP":
        return [vp, vs, rho * vp]
    return [vp, vs, rho * vs]


def padded_shape(dims):
    nz, nx, nPml, nPad = dims
    return nz + 2 * nPml + nPad, nx + 2 * nPml


def random_mask(rng, dims):
    """uniform in [0, 1] with a row of exact 0 (the first) and, where there is room, a row of exact 1 (the last)"""
    m = rng.uniform(0.0, 1.0, padded_shape(dims)).astype(np.float32)
    m[0, :] = 0.0
    if m.shape[0] >= 3:
        m[-1, :] = 1.0
    return m


def interior_mask(dims):
    nz, nx, nPml, _ = dims
    m = np.zeros(padded_shape(dims), np.float32)
    m[nPml:nPml + nz, nPml:nPml + nx] = 1.0
    return m


def make_module(cls_name, dims, f, mask, dtype=torch.float32, device="cpu", para_fname="unused.json", Stf=None, grads=(True, True, True)):
    """the module at the fields f, its reference model 3 % off so that the blend matters (as tests/test_gpu_param_maps.py builds it)"""
    nz, nx, nPml, nPad = dims
    opt = dict(nz=nz, nx=nx, nz_orig=nz, nx_orig=nx, nPml=nPml, nPad=nPad, para_fname=para_fname)
    T = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype, device=device)
    ref = [T(np.asarray(a, np.float32) * np.float32(1.03)) for a in f]      # float32 values too: both precisions see the same inputs
    mod = getattr(M, cls_name)(ref[0], ref[1], ref[2], Stf, opt, Mask=torch.tensor(mask, dtype=dtype, device=device))
    for n, a, g in zip(mod.NAMES, f, grads):
        t = T(np.asarray(a, np.float32))      # the float32 values, in either precision
        setattr(mod, n, torch.nn.Parameter(t) if g else t)
    return mod


def chain64(mod64):
    """the module's own expression on a float64 module, as a function of the three fields"""
    def f(a, b, c):
        pad = ft.padding(a, b, c, mod64.nz_orig, mod64.nx_orig, mod64.nz, mod64.nx, mod64.nPml, mod64.nPad)
        return mod64.lame(*[mod64.Mask * p + (1.0 - mod64.Mask) * getattr(mod64, n + "_ref") for n, p in zip(mod64.NAMES, pad)])
    return f


def tangent64(mod64, v):
    """float64 torch.func.jvp of the same expression -> three numpy arrays on the padded grid"""
    cur = tuple(getattr(mod64, n).detach() for n in mod64.NAMES)
    v = tuple(torch.as_tensor(np.asarray(a, np.float64)) for a in v)
    return [t.numpy() for t in torch.func.jvp(chain64(mod64), cur, v)[1]]


def jacobian64(mod64):
    """dense float64 Jacobian of the chain, (3 nzp nxp, 3 nz nx)"""
    cur = [getattr(mod64, n).detach() for n in mod64.NAMES]
    n = cur[0].numel()
    f = chain64(mod64)
    flat = lambda x: torch.cat([t.reshape(-1) for t in f(*[x[k * n:(k + 1) * n].reshape(cur[0].shape) for k in range(3)])])
    return torch.autograd.functional.jacobian(flat, torch.cat([t.reshape(-1) for t in cur])).numpy()


def diag64(mod64, h):
    """diag(J^T diag(h) J) from the dense Jacobian -> three (nz, nx) arrays"""
    J = jacobian64(mod64)
    hh = np.concatenate([np.asarray(a, np.float64).ravel() for a in h])
    d = (J * J * hh[:, None]).sum(0)
    shp = tuple(getattr(mod64, mod64.NAMES[0]).shape)
    return [d[k * shp[0] * shp[1]:(k + 1) * shp[0] * shp[1]].reshape(shp) for k in range(3)]


def noise_v(rng, f, rel=0.01):
    """1 % noise on each field, float32"""
    return [(rel * np.asarray(a) * rng.uniform(-1.0, 1.0, np.shape(a))).astype(np.float32) for a in f]


def inputs(cls_name, dims, seed=SEED):
    """-> fields f (float64), Mask, a tangent v (1 % noise), weights w and a non-negative diagonal h on the padded grid (float32)"""
    rng = np.random.default_rng([seed, CLASSES.index(cls_name), *dims])
    f = fields(cls_name, rng, dims[0], dims[1])
    mask = random_mask(rng, dims)
    v = noise_v(rng, f)
    w = [rng.standard_normal(padded_shape(dims)).astype(np.float32) for _ in range(3)]
    h = [rng.uniform(0.0, 1.0, padded_shape(dims)).astype(np.float32) for _ in range(3)]
    return f, mask, v, w, h


def close(got, ref, tol, what):
    """every array within tol of ITS largest reference entry; prints the measured figure first"""
    devs = []
    for g, r in zip(got, ref):
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        scale = np.abs(r).max()
        assert scale > 0 and np.isfinite(g).all(), what
        devs.append(float(np.abs(g - r).max() / scale))
    print("param tangent %s: max deviation / max |reference| per array %s (bound %.0e)" % (what, ["%.1e" % d for d in devs], tol))
    assert max(devs) <= tol, (what, devs)
    return devs


def holder_bound(tol, Pv, w, Ptw, v):
    """the Hoelder sum of the two per-array bounds for <P v, w> - <v, P^T w>"""
    f = lambda a: np.asarray(a, np.float64)
    return (tol * sum(np.abs(f(a)).max() * np.abs(f(b)).sum() for a, b in zip(Pv, w))
            + tol * sum(np.abs(f(a)).max() * np.abs(f(b)).sum() for a, b in zip(Ptw, v)))


def dot(a, b):
    return sum(float((np.asarray(x, np.float64) * np.asarray(y, np.float64)).sum()) for x, y in zip(a, b))
