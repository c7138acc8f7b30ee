"""The smoothing operator's yardstick (inputs and mathematics only): the operator of include/sepfwi.h (sepfwi_smooth_apply) exactly as it
is defined, as one dense float64 numpy matrix per row (x) and per column (z) -- nothing is restated as a gather.  Plus the seeded cases
that the host and the GPU tests share (every input is born float32 and up-cast for the reference, so input rounding is part of no
deviation) and ctypes callers of the two C-ABI entry points for numpy arrays or HIP tensors."""
import ctypes as C

import numpy as np
import torch

# (nz, nx, rz, rx): a single row; radii that are no multiple of anything; a radius beyond the grid; several tiles both ways
GRIDS = [(1, 64, 5, 5), (5, 65, 7, 32), (67, 9, 32, 3), (4, 129, 2, 12), (3, 63, 64, 64), (300, 500, 24, 24)]
SMALL = GRIDS[:5]
WIDTHS = ("constant", "random", "zero_patch", "x_null", "z_null")
U = 2.0 ** -24


def taps(grid):
    """T of the bounds: (2 rx + 1) + (2 rz + 1)"""
    return (2 * grid[3] + 1) + (2 * grid[2] + 1)


def widths(grid, kind, seed=0):
    """-> sigx, sigz: float32 (nz, nx) arrays in cells, or None for an identity axis"""
    nz, nx, rz, rx = grid
    rng = np.random.default_rng(100003 * nz + 101 * nx + 7 * rz + rx + 7919 * seed + 31 * WIDTHS.index(kind))
    if kind == "constant":
        sx, sz = np.full((nz, nx), rx / 3.0), np.full((nz, nx), rz / 3.0)
    else:       # up to r / 2 + 0.5: the outermost tap carries weight >= 1 / e in places
        sx, sz = rng.uniform(0.0, rx / 2.0 + 0.5, (nz, nx)), rng.uniform(0.0, rz / 2.0 + 0.5, (nz, nx))
    if kind == "zero_patch":        # wide cells with a patch of exact zeros among them
        sx[:], sz[:] = rx / 2.0 + 0.5, rz / 2.0 + 0.5
        sx[nz // 3:nz // 3 + max(1, nz // 4), nx // 3:nx // 3 + max(2, nx // 4)] = 0.0
        sz[nz // 3:nz // 3 + max(1, nz // 4), nx // 3:nx // 3 + max(2, nx // 4)] = 0.0
    sx, sz = sx.astype(np.float32), sz.astype(np.float32)
    return (None if kind == "x_null" else sx), (None if kind == "z_null" else sz)


def fields(grid, seed=0, present=(1, 1, 1)):
    """three float32 (nz, nx) fields of the sizes of Vp, Vs and density updates (None where `present` has 0)"""
    rng = np.random.default_rng(1000 * grid[0] + grid[1] + 104729 * seed)
    out = []
    for b, on in zip((300.0, -170.0, 24.0), present):
        a = (b * (0.3 + rng.standard_normal(grid[:2]))).astype(np.float32)
        out.append(a if on else None)
    return out


# ---- the definition, float64, dense -------------------------------------------------------------------------------------------------
def kernel_matrix(sig, r):
    """K of one row or column, dense: sig the float64 widths along it -- or, for sig of shape (lines, n), one K per line"""
    sig = np.asarray(sig, np.float64)
    single = sig.ndim == 1
    q = np.atleast_2d(sig) ** 2
    c, n = q.shape
    idx = np.arange(n)
    K = np.zeros((c, n, n))
    K[:, idx, idx] = 1.0
    for t in range(1, min(r, n - 1) + 1):          # the two diagonals at distance t
        d = q[:, :-t] + q[:, t:]
        on = d > 0
        w = np.where(on, np.exp(-float(t * t) / np.where(on, d, 1.0)), 0.0)
        K[:, idx[:-t], idx[t:]] = w
        K[:, idx[t:], idx[:-t]] = w
    return K[0] if single else K


def _axis(u, sig, r, axis, transpose):
    """Sx (axis 1) or Sz (axis 0), or its transpose, of the float64 fields u of shape (nz, nx, F)"""
    if sig is None or r == 0:
        return u.copy()
    sig = sig.astype(np.float64)
    lines = u if axis == 1 else u.transpose(1, 0, 2)
    sg = sig if axis == 1 else sig.T
    out = np.empty(lines.shape)
    for i in range(0, lines.shape[0], 16):         # 16 lines' matrices at a time
        K = kernel_matrix(sg[i:i + 16], r)
        N = K.sum(axis=2)[:, :, None]
        out[i:i + 16] = K @ (lines[i:i + 16] / N) if transpose else (K @ lines[i:i + 16]) / N
    return out if axis == 1 else out.transpose(1, 0, 2).copy()


def _stack(us):
    us = [us] if isinstance(us, np.ndarray) else list(us)
    return np.stack([np.asarray(a, np.float64) for a in us], axis=2)


def S(us, grid, sigx, sigz):
    """S u = Sx Sz u of one field or of a list of fields -> a field, or a list"""
    out = _axis(_axis(_stack(us), sigz, grid[2], 0, False), sigx, grid[3], 1, False)
    return out[:, :, 0].copy() if isinstance(us, np.ndarray) else [out[:, :, k].copy() for k in range(out.shape[2])]


def St(ys, grid, sigx, sigz):
    """S^T y = Sz^T Sx^T y"""
    out = _axis(_axis(_stack(ys), sigx, grid[3], 1, True), sigz, grid[2], 0, True)
    return out[:, :, 0].copy() if isinstance(ys, np.ndarray) else [out[:, :, k].copy() for k in range(out.shape[2])]


_CACHE = {}


def reference(grid, kind, seed=0):
    """-> dict(S=[S u_k], St=[S^T u_k], Sabs=[S |u_k|], Stabs=[S^T |u_k|]) of the three fields of `fields(grid, seed)`, computed once
    and read-only"""
    if (grid, kind, seed) not in _CACHE:      # the seeds 0 and 1 share the lines' matrices: one sweep for both
        sx, sz = widths(grid, kind)
        u = fields(grid, 0) + fields(grid, 1)
        fwd, bwd = S(u + [np.abs(a) for a in u], grid, sx, sz), St(u + [np.abs(a) for a in u], grid, sx, sz)
        for a in fwd + bwd:
            a.setflags(write=False)
        for sd in (0, 1):
            at = lambda x, first: x[first + 3 * sd:first + 3 * sd + 3]
            _CACHE[(grid, kind, sd)] = dict(S=at(fwd, 0), Sabs=at(fwd, 6), St=at(bwd, 0), Stabs=at(bwd, 6))
    return _CACHE[(grid, kind, seed)]


def smoother_of(grid, kind, radius="table"):
    """sepfwi.smooth.Smoother of the case, widths in cells"""
    from sepfwi.smooth import Smoother
    sx, sz = widths(grid, kind)
    t = lambda a: None if a is None else torch.tensor(a)
    return Smoother(grid[:2], t(sx), t(sz), unit="cells", radius=(grid[3], grid[2]) if radius == "table" else radius)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def _ptr(a):
    if a is None:
        return None
    return C.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a.ctypes.data_as(C.c_void_p)


def _triple(arrs):
    return (C.c_void_p * 3)(*[None if a is None else _ptr(a).value for a in arrs])


def _put(a, on_device):
    if a is None:
        return None
    return torch.tensor(a).cuda() if on_device else np.ascontiguousarray(a, np.float32)


def _like(a, on_device):
    if a is None:
        return None
    return torch.empty(a.shape, dtype=torch.float32, device="cuda") if on_device else np.empty(a.shape, np.float32)


def host(a):
    return None if a is None else (a.cpu().numpy() if torch.is_tensor(a) else a)


def c_plan(L, grid, sigx, sigz, on_device=False, inv=("auto", "auto")):
    """sepfwi_smooth_plan -> rc, (sigx, sigz, inv_nx, inv_nz) as the call saw them (numpy arrays or HIP tensors; keep them alive)"""
    nz, nx, rz, rx = grid
    sx, sz = _put(sigx, on_device), _put(sigz, on_device)
    ix = _like(sigx, on_device) if inv[0] == "auto" else inv[0]
    iz = _like(sigz, on_device) if inv[1] == "auto" else inv[1]
    rc = L.sepfwi_smooth_plan(int(nz), int(nx), int(rx), int(rz), _ptr(sx), _ptr(sz), _ptr(ix), _ptr(iz), None)
    return rc, (sx, sz, ix, iz)


def c_apply(L, grid, plan, u, transpose, on_device=False, in_place=False):
    """sepfwi_smooth_apply on host arrays or HIP tensors -> rc, outputs as float32 numpy (None for a NULL field)"""
    nz, nx, rz, rx = grid
    src = [_put(None if a is None else a.copy(), on_device) for a in u]
    dst = src if in_place else [_like(a, on_device) for a in u]
    rc = L.sepfwi_smooth_apply(int(nz), int(nx), int(rx), int(rz), *[_ptr(a) for a in plan], 1 if transpose else 0, _triple(src), _triple(dst), None)
    if on_device:
        torch.cuda.synchronize()
    return rc, [host(a) for a in dst]
