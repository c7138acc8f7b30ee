"""A model-space smoothing operator S with its exact transpose (an unpinned extension: the reference has nothing of the kind): a separable,
normalised Gaussian, truncated at a radius, whose width may vary from cell to cell.  With the widths in cells, along x in row i

    Kx[j, m] = 1 for m = j,   exp(-(m - j)^2 / (sigx[i,j]^2 + sigx[i,m]^2)) for 0 < |m - j| <= rx inside the grid (0 where the sum of
               squares is not > 0),   0 everywhere else
    Nx[i,j]  = sum_m Kx[j, m],      Sx u = (Kx u) / Nx,      Sx^T y = Kx (y / Nx)

the same down every column with sigz, rz, and S = Sx Sz, S^T = Sz^T Sx^T (include/sepfwi.h, sepfwi_smooth_apply, has it written out).
S keeps constants, is the identity where the widths are 0, and <S u, y> = <u, S^T y> exactly, so S S^T is a symmetric non-negative
preconditioner for conjugate gradients and p = p_ref + s S y a change of variables whose gradient is s S^T g:

    sm = Smoother.from_wavelength(fwi, vs, fmax=12.0)                    # sigma = half the shortest S wavelength
    g = sm.apply_t(sm.apply(grads))                                      # a smoothed gradient (S S^T g: still a descent direction)
    p, hist = gauss_newton_cg(hessvec, g, diag=D, precond=sm.preconditioner(D))
    obj = PyTorchObjective(fwi, loss, smoother=sm)                       # L-BFGS in y, the model p_ref + s S y

On HIP float32 tensors one application to three fields is two launches (csrc/smoother.hip); on CPU tensors or float64 tensors the same
definition runs in torch.  The operator acts on the model only: under sepfwi.dist every rank applies it after the gradient all-reduce.
"""
from __future__ import annotations

import math

import torch

from . import _native
from . import utils as _utils

MAX_RADIUS = 64


def _axis_pass(u, sig, inv, r, dim, transpose):
    """(K u) inv (forward) or K (u inv) (transpose) along `dim` of the 2-D tensor u, in u's dtype: the definition, pair by pair"""
    v = u * inv if transpose else u
    acc = v.clone()
    q = sig * sig
    n = u.shape[dim]
    for t in range(1, min(r, n - 1) + 1):
        lo, hi = slice(0, n - t), slice(t, n)
        a, b = ((slice(None), lo), (slice(None), hi)) if dim == 1 else ((lo, slice(None)), (hi, slice(None)))
        d = q[a] + q[b]
        w = torch.where(d > 0, torch.exp(-float(t * t) / d), torch.zeros_like(d))
        lower, upper = w * v[b], w * v[a]
        acc[a] += lower
        acc[b] += upper
    return acc if transpose else acc * inv


class _SmoothFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sm, u):
        ctx.sm = sm
        return sm.apply((u.detach(),))[0]

    @staticmethod
    def backward(ctx, grad):
        return None, ctx.sm.apply_t((grad,))[0]


class Smoother(object):
    """module_or_shape: a parameterisation module (its fields' shape; dx, dz of its parameter file) or (nz, nx).  sigma_x, sigma_z: a
    non-negative number or (nz, nx) tensor, in metres (unit="m", divided by dx / dz) or in cells (unit="cells"); None: that axis is the
    identity.  radius: None (min(64, ceil(3 max sigma)) per axis, in cells), an int for both axes or (rx, rz)."""

    def __init__(self, module_or_shape, sigma_x, sigma_z, dx=None, dz=None, unit="m", radius=None):
        if unit not in ("m", "cells"):
            raise ValueError("Smoother: unit must be 'm' or 'cells'")
        if isinstance(module_or_shape, (tuple, list, torch.Size)):
            self.module, self.names = None, None
            shape = tuple(int(x) for x in module_or_shape)
        else:
            self.module = module_or_shape
            self.names = tuple(self.module.NAMES)
            shape = tuple(next(iter(self.module.parameters())).shape)
        if len(shape) != 2 or min(shape) < 1:
            raise ValueError("Smoother: the fields must have a shape (nz, nx)")
        self.shape = shape
        if unit == "m" and (dx is None or dz is None):
            if self.module is None or getattr(self.module, "para_fname", None) is None:
                raise ValueError("Smoother: widths in metres need dx and dz (or a module with a parameter file)")
            para = _utils.read_para(self.module.para_fname)
            dx, dz = (para["dx"] if dx is None else dx), (para["dz"] if dz is None else dz)
        self.dx, self.dz = (1.0, 1.0) if unit == "cells" else (float(dx), float(dz))
        if not (self.dx > 0 and self.dz > 0 and math.isfinite(self.dx) and math.isfinite(self.dz)):
            raise ValueError("Smoother: dx and dz must be positive")

        def cells(sigma, h, what):
            if sigma is None:
                return None
            s = sigma.detach().to(device="cpu", dtype=torch.float64) if torch.is_tensor(sigma) else torch.full(shape, float(sigma), dtype=torch.float64)
            if tuple(s.shape) != shape:
                raise ValueError("Smoother: %s must be a number or a tensor of shape %s" % (what, shape))
            if not bool(torch.isfinite(s).all()) or bool((s < 0).any()):
                raise ValueError("Smoother: %s must be finite and non-negative" % what)
            return (s / h).to(torch.float32).contiguous()      # the widths every path starts from: float32, in cells
        self.sigma = (cells(sigma_x, self.dx, "sigma_x"), cells(sigma_z, self.dz, "sigma_z"))
        if radius is None:
            radius = tuple(0 if s is None else min(MAX_RADIUS, int(math.ceil(3.0 * float(s.max())))) for s in self.sigma)
        elif isinstance(radius, (tuple, list)):
            radius = tuple(int(r) for r in radius)
        else:
            radius = (int(radius), int(radius))
        if len(radius) != 2 or not all(0 <= r <= MAX_RADIUS for r in radius):
            raise ValueError("Smoother: a radius must lie between 0 and %d" % MAX_RADIUS)
        self.radius = radius            # (rx, rz)
        self._plans = {}                # (device, dtype) -> (sigx, sigz, inv_nx, inv_nz) there; HIP float32: planned by the library
        self.plan(torch.device("cpu"), torch.float32)

    @classmethod
    def from_wavelength(cls, module, vs, fmax, fraction=0.5, **kw):
        """sigma = fraction vs / fmax on both axes: a share of the shortest wavelength in the band, cell by cell.  vs: a number or an
        (nz, nx) tensor in m/s, fmax in Hz."""
        if not (fmax > 0 and fraction >= 0):
            raise ValueError("from_wavelength: fmax must be positive and fraction non-negative")
        sigma = (vs.detach().double() if torch.is_tensor(vs) else float(vs)) * (float(fraction) / float(fmax))
        return cls(module, sigma, sigma, unit="m", **kw)

    # -- public ----------------------------------------------------------------------------------------------------------------------
    def apply(self, fields):
        """S on every tensor of the tuple `fields` (module.NAMES order; None entries are passed through)"""
        return self._run(fields, False)

    def apply_t(self, fields):
        """S^T on every tensor of the tuple"""
        return self._run(fields, True)

    def gram(self, fields):
        """S S^T on every tensor of the tuple: symmetric and non-negative"""
        return self._run(self._run(fields, True), False)

    def __call__(self, tensor):
        """S tensor, differentiable: the backward is S^T"""
        return _SmoothFunction.apply(self, tensor)

    def preconditioner(self, diag=None):
        """-> a callable r -> D^-1/2 S S^T D^-1/2 r on tuples of tensors, for gauss_newton_cg(precond=): symmetric and non-negative.
        diag: None (D = I) or a tuple of non-negative tensors such as the pseudo-Hessian, floored as gauss_newton_cg floors its Jacobi
        diagonal (negative entries 0, then 1e-12 of the largest)."""
        if diag is None:
            return lambda r: list(self.gram(tuple(r)))
        scale = []
        for d in diag:
            if d is None:
                scale.append(None)
                continue
            d = d.detach().clamp_min(0)
            scale.append(torch.rsqrt(d.clamp_min(1e-12 * float(d.max()) if float(d.max()) > 0 else 1.0)))
        mul = lambda ts: tuple(None if t is None else (t if s is None else t * s.to(device=t.device, dtype=t.dtype)) for t, s in zip(ts, scale))
        return lambda r: list(mul(self.gram(mul(tuple(r)))))

    def plan(self, device, dtype):
        """the widths and 1 / Nx, 1 / Nz on `device` in `dtype`, made once: -> (sigx, sigz, inv_nx, inv_nz), None for an identity axis"""
        key = (torch.device(device), dtype)
        if key in self._plans:
            return self._plans[key]
        fused = key[0].type == "cuda" and dtype == torch.float32
        sig = [None if s is None else s.to(device=key[0], dtype=dtype).contiguous() for s in self.sigma]
        if fused:
            inv = [None if s is None else torch.empty_like(s) for s in sig]
            ptr = _native.ptr
            _native.check(_native.lib().sepfwi_smooth_plan(self.shape[0], self.shape[1], self.radius[0], self.radius[1], ptr(sig[0]), ptr(sig[1]),
                                                           ptr(inv[0]), ptr(inv[1]), _native.stream_arg(key[0])))
        else:
            one = torch.ones(self.shape, dtype=dtype, device=key[0])
            inv = [None if s is None else 1.0 / _axis_pass(one, s, one, r, dim, True) for s, r, dim in zip(sig, self.radius, (1, 0))]      # N = K 1
        self._plans[key] = (sig[0], sig[1], inv[0], inv[1])
        return self._plans[key]

    # -- the two paths ---------------------------------------------------------------------------------------------------------------
    def _run(self, fields, transpose):
        if torch.is_tensor(fields):
            raise ValueError("Smoother: apply, apply_t and gram take a tuple of fields (None: passed through); S of one tensor is smoother(tensor)")
        fields = tuple(fields)
        for t in fields:
            if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != self.shape):
                raise ValueError("Smoother: every field must be a tensor of shape %s (or None)" % (self.shape,))
        out = [None] * len(fields)
        fused = {}      # device -> the indices of its HIP float32 fields
        for k, t in enumerate(fields):
            if t is None:
                continue
            if t.is_cuda and t.dtype == torch.float32:
                fused.setdefault(t.device, []).append(k)
            else:
                out[k] = self._torch_apply(t.detach(), transpose)
        for dev, idx in fused.items():
            for at in range(0, len(idx), 3):
                part = idx[at:at + 3]
                for k, o in zip(part, self._launch([fields[k].detach().contiguous() for k in part], transpose)):
                    out[k] = o
        return tuple(out)

    def _launch(self, ts, transpose):
        """one call of sepfwi_smooth_apply for up to three HIP float32 fields of one device"""
        dev = ts[0].device
        sigx, sigz, invx, invz = self.plan(dev, torch.float32)
        outs = [torch.empty_like(t) for t in ts]
        ptr, triple = _native.ptr, _native.triple
        _native.check(_native.lib().sepfwi_smooth_apply(self.shape[0], self.shape[1], self.radius[0], self.radius[1], ptr(sigx), ptr(sigz),
                                                        ptr(invx), ptr(invz), 1 if transpose else 0, triple(ts), triple(outs),
                                                        _native.stream_arg(dev)))
        return outs

    def _torch_apply(self, u, transpose):
        sigx, sigz, invx, invz = self.plan(u.device, u.dtype)
        passes = [(sigx, invx, self.radius[0], 1), (sigz, invz, self.radius[1], 0)]       # S^T = Sz^T Sx^T: x first
        if not transpose:
            passes.reverse()                                                                # S = Sx Sz: z first
        out = u
        for sig, inv, r, dim in passes:
            if sig is not None and r > 0:
                out = _axis_pass(out, sig, inv, r, dim, transpose)
        return out.clone() if out is u else out
