"""The model regulariser's yardstick (inputs and mathematics only): the functional of include/sepfwi.h (sepfwi_regularizer) exactly as it
is defined, in float64 torch -- the value as written, the gradient by torch.autograd.grad, the product by
torch.autograd.functional.hvp; nothing is restated in gather form.  Plus the seeded cases that the host and the GPU tests share (every
input is born float32 and up-cast for the reference, so input rounding is part of no deviation), the float32 torch fallback of
sepfwi.regularize on a stand-in module, and a ctypes caller of the two C-ABI entry points for numpy arrays or HIP tensors."""
import ctypes as C

import numpy as np
import torch

GRIDS = [(1, 1), (1, 65), (7, 1), (2, 2), (5, 63), (64, 64), (33, 129), (130, 257)]
DX, DZ = np.float32(10.0), np.float32(7.5)
NAMES = ("A", "B", "C")
BASE = (3000.0, 1700.0, 2400.0)          # the three fields are of the sizes of Vp, Vs and density
# the typical |grad p| / s of `fields` is 1e-3 .. 1e-2: eps 1e-1 is large against it (TV acts as Tikhonov), 1e-5 small (nearly |grad p|)
EPS, EPS_LARGE, EPS_SMALL = np.float32(2e-3), np.float32(1e-1), np.float32(1e-5)
F32 = lambda *x: np.array(x, dtype=np.float32)
CASES = {
    "full": dict(),
    "no_weight": dict(weight=False),
    "null_field": dict(null=1),
    "alpha_only": dict(beta=F32(0, 0, 0), gamma=F32(0, 0, 0)),
    "beta_only": dict(alpha=F32(0, 0, 0), gamma=F32(0, 0, 0)),
    "gamma_only": dict(alpha=F32(0, 0, 0), beta=F32(0, 0, 0)),
    "eps_large": dict(eps=EPS_LARGE),
    "eps_small": dict(eps=EPS_SMALL),
}


def fields(grid, seed=0):
    """-> p, p0, v (three (nz, nx) float32 arrays each) and W with about 20 % exact zeros"""
    rng = np.random.default_rng(1000 * grid[0] + grid[1] + 7919 * seed)
    p, p0, v = [], [], []
    for b in BASE:
        a = b * (1.0 + 0.05 * rng.standard_normal(grid))
        a[grid[0] // 2:, grid[1] // 3:] += 0.08 * b          # an edge, for the total variation
        p.append(a.astype(np.float32))
        p0.append((a + 0.03 * b * rng.standard_normal(grid)).astype(np.float32))
        v.append((0.02 * b * rng.standard_normal(grid)).astype(np.float32))
    W = (rng.uniform(0.5, 1.5, grid) * (rng.uniform(size=grid) > 0.2)).astype(np.float32)
    return p, p0, v, W


def case(grid, name, seed=0):
    """every argument of sepfwi_regularizer for one case, as float32 numpy (None: a NULL pointer)"""
    kw = CASES[name]
    p, p0, v, W = fields(grid, seed)
    c = dict(nz=grid[0], nx=grid[1], dx=DX, dz=DZ, p=p, p0=p0, v=v, W=W if kw.get("weight", True) else None,
             alpha=kw.get("alpha", F32(0.7, 0.0, 1.3)), beta=kw.get("beta", F32(0.4, 0.9, 0.0)), gamma=kw.get("gamma", F32(0.0, 0.6, 1.1)),
             scale=F32(3100.0, 1650.0, 2500.0), eps=kw.get("eps", EPS))
    if "null" in kw:
        for key in ("p", "p0", "v"):
            c[key][kw["null"]] = None
    return c


# ---- the definition, float64 --------------------------------------------------------------------------------------------------------
def value64(p, c):
    """R of the case c at the float64 tensors p (None: a skipped field), as written in include/sepfwi.h"""
    W = 1.0 if c["W"] is None else torch.tensor(c["W"].astype(np.float64))
    dx, dz, eps = float(c["dx"]), float(c["dz"]), float(c["eps"])
    total = torch.zeros((), dtype=torch.float64)
    for k, pk in enumerate(p):
        if pk is None:
            continue
        s, al, be, ga = (float(c[key][k]) for key in ("scale", "alpha", "beta", "gamma"))
        gx, gz = torch.zeros_like(pk), torch.zeros_like(pk)
        gx[:, :-1] = (pk[:, 1:] - pk[:, :-1]) / (s * dx)
        gz[:-1, :] = (pk[1:, :] - pk[:-1, :]) / (s * dz)
        n2 = gx ** 2 + gz ** 2
        cell = 0.5 * be * n2
        if al > 0:
            cell = cell + 0.5 * al * ((pk - torch.tensor(c["p0"][k].astype(np.float64))) / s) ** 2
        if ga > 0:
            cell = cell + ga * (torch.sqrt(n2 + eps ** 2) - eps)
        total = total + (W * cell).sum()
    return total


def _up(arrs):
    return [None if a is None else torch.tensor(a.astype(np.float64)) for a in arrs]


def reference(c):
    """-> value (float), gradient and product (lists of float64 numpy arrays, None for a skipped field)"""
    p, v = _up(c["p"]), _up(c["v"])
    on = [k for k in range(3) if p[k] is not None]
    leaves = [p[k].clone().requires_grad_(True) for k in on]
    put = lambda ts: [ts[on.index(k)] if k in on else None for k in range(3)]
    val = value64(put(leaves), c)
    g = torch.autograd.grad(val, leaves, allow_unused=True)
    hv = torch.autograd.functional.hvp(lambda *ts: value64(put(list(ts)), c), tuple(p[k] for k in on), tuple(v[k] for k in on))[1]
    full = lambda ts: [None if k not in on else (np.zeros((c["nz"], c["nx"])) if ts[on.index(k)] is None else ts[on.index(k)].detach().numpy()) for k in range(3)]
    return float(val.detach()), full(g), full(hv)


def share(got, ref):
    """an array's largest deviation as a share of the reference array's largest entry (0 / 0 = 0: both must be exactly zero)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    top, dev = np.abs(ref).max(), np.abs(got - ref).max()
    return 0.0 if dev == 0.0 else (np.inf if top == 0.0 else dev / top)


# ---- sepfwi.regularize on a stand-in module -----------------------------------------------------------------------------------------
class Fields(torch.nn.Module):
    """three (nz, nx) fields under the names of a parameterisation module; None: a field that is not inverted"""
    NAMES = NAMES
    para_fname = None

    def __init__(self, arrs, dtype, device="cpu", shape=None):
        super().__init__()
        for n, a in zip(NAMES, arrs):
            if a is None:
                setattr(self, n, torch.zeros(shape, dtype=dtype, device=device))
            else:
                setattr(self, n, torch.nn.Parameter(torch.tensor(a).to(device=device, dtype=dtype)))


def regularizer_of(c, dtype, device="cpu"):
    """-> (module, Regularizer) of the case c on tensors of `dtype`: float32 / float64 on the CPU are the torch fallback"""
    from sepfwi.regularize import Regularizer
    mod = Fields(c["p"], dtype, device, (c["nz"], c["nx"]))
    d = lambda key: {n: float(c[key][k]) for k, n in enumerate(NAMES)}
    prior = {n: torch.tensor(a) for n, a in zip(NAMES, c["p0"]) if a is not None}
    reg = Regularizer(mod, alpha=d("alpha"), beta=d("beta"), gamma=d("gamma"), eps=float(c["eps"]), prior=prior, scale=d("scale"),
                      weight=None if c["W"] is None else torch.tensor(c["W"]), dx=float(c["dx"]), dz=float(c["dz"]))
    return mod, reg


def fallback(c, dtype=torch.float32):
    """value, gradient, product of the torch path of sepfwi.regularize on CPU tensors of `dtype`, shaped as `reference` returns them"""
    mod, reg = regularizer_of(c, dtype)
    assert not reg._fusable([getattr(mod, n).detach() for n in reg.active])
    val, g = reg.value_and_grad()
    hv = reg.hvp(tuple(None if a is None else torch.tensor(a).to(dtype) for a in c["v"]))
    out = lambda ts: [None if t is None else t.detach().numpy() for t in ts]
    return float(val), out(g), out(hv)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def _ptr(a):
    if a is None:
        return None
    return C.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a.ctypes.data_as(C.c_void_p)


def _triple(arrs):
    return (C.c_void_p * 3)(*[None if a is None else _ptr(a).value for a in arrs])


def _model_args(c, on_device):
    put = (lambda a: None if a is None else torch.tensor(a).cuda()) if on_device else (lambda a: None if a is None else np.ascontiguousarray(a))
    keep = dict(p=[put(a) for a in c["p"]], p0=[put(a) for a in c["p0"]], W=put(c["W"]), v=[put(a) for a in c["v"]])
    f3 = lambda a: (C.c_float * 3)(*[float(x) for x in a])
    args = [int(c["nz"]), int(c["nx"]), float(c["dx"]), float(c["dz"]), _triple(keep["p"]), _triple(keep["p0"]), _ptr(keep["W"]),
            f3(c["alpha"]), f3(c["beta"]), f3(c["gamma"]), f3(c["scale"]), float(c["eps"])]
    return keep, args


def _empty(like, on_device):
    return [None if a is None else (torch.empty(a.shape, dtype=torch.float32, device="cuda") if on_device else np.empty(a.shape, np.float32)) for a in like]


def _host(arrs):
    return [None if a is None else (a.cpu().numpy() if torch.is_tensor(a) else a) for a in arrs]


def c_value_grad(L, c, on_device=False, device_value=False):
    """sepfwi_regularizer on host arrays or HIP tensors -> rc, value (float), g (numpy float32, None for a skipped field)"""
    keep, args = _model_args(c, on_device)
    g = _empty(c["p"], on_device)
    if device_value:
        val = torch.full((), -1.0, dtype=torch.float64, device="cuda")
        rc = L.sepfwi_regularizer(*args, _ptr(val), _triple(g), None)
        return rc, float(val), _host(g)
    val = C.c_double(-1.0)
    rc = L.sepfwi_regularizer(*args, C.cast(C.byref(val), C.c_void_p), _triple(g), None)
    return rc, val.value, _host(g)


def c_hvp(L, c, on_device=False):
    keep, args = _model_args(c, on_device)
    hv = _empty(c["p"], on_device)
    rc = L.sepfwi_regularizer_hvp(*args, _triple(keep["v"]), _triple(hv), None)
    return rc, _host(hv)
