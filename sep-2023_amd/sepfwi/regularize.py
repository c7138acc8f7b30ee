"""Model regularisation for the parameterisation modules: damping towards a prior, first-order Tikhonov and Charbonnier-smoothed
isotropic total variation of the inverted fields, with the gradient and the exact Hessian-vector product (an extension without a
counterpart in the reference, whose objective has data terms only).  For each inverted field p of shape (nz, nx), with its prior p0,
a scale s, cell weights W and the grid spacings dx, dz:

    q = (p - p0) / s,   gx = (p(i,j+1) - p(i,j)) / (s dx),   gz = (p(i+1,j) - p(i,j)) / (s dz)     (0 in the last column / row)
    R(p) = sum over the cells of  W [ alpha q^2 / 2 + beta (gx^2 + gz^2) / 2 + gamma (sqrt(gx^2 + gz^2 + eps^2) - eps) ]

and the total is the sum over the fields (include/sepfwi.h, sepfwi_regularizer, has the gradient and the product written out).  R is
convex, so its Hessian is symmetric and non-negative: adding `hvp` to a Gauss-Newton product with the exact adjoint keeps what
conjugate gradients need.

    reg = Regularizer(fwi, beta=1e-3, gamma={"Den": 1e-2})
    loss = fwi(ids) + reg()                                     # under PyTorchObjective / minimize_lbfgsb, unchanged
    obj = PyTorchObjective(fwi, lambda: fwi(ids) + reg(), shot_ids=ids, regularizer=reg)      # hessp carries reg.hvp
    p, hist = gauss_newton_cg(lambda v: add(fwi.gauss_newton(v, ids, exact=True), reg.hvp(v)), grad)

On HIP float32 tensors value and gradient are ONE launch over the fields (plus a one-block sum), the product another
(csrc/regularizer.hip); on CPU tensors -- the modules "exactly like the reference" -- or float64 tensors the same expressions run in
torch.  The regulariser is a function of the model only: under sepfwi.dist every rank adds the same term AFTER the gradient all-reduce,
because it attaches to the parameter leaves and not to the operator, whose backward is what the all-reduce sums.  Nothing in dist.py
knows of it.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native
from . import utils as _utils

USE_FUSED = True   # tests switch it off to compare the fused launches with the torch expressions


def _diff(a, rx, rz):
    gx, gz = torch.zeros_like(a), torch.zeros_like(a)
    gx[:, :-1] = (a[:, 1:] - a[:, :-1]) * rx
    gz[:-1, :] = (a[1:, :] - a[:-1, :]) * rz
    return gx, gz


def _gather(t0, fx, fz, rx, rz):
    """t0 - fx rx - fz rz + fx(i, j-1) rx + fz(i-1, j) rz: the transpose of `_diff` applied to a flux (0 in its last column / row)"""
    out = (t0 - fx * rx) - fz * rz
    out[:, 1:] += fx[:, :-1] * rx
    out[1:, :] += fz[:-1, :] * rz
    return out


class _RegFunction(torch.autograd.Function):
    """forward keeps the gradient that the one launch computed with the value; backward scales it by the incoming scalar."""

    @staticmethod
    def forward(ctx, reg, *fields):
        value, grads = reg._value_and_grad([t.detach() for t in fields])
        ctx.grads = grads
        return value.to(fields[0].dtype)

    @staticmethod
    def backward(ctx, grad_value):
        return (None,) + tuple(g * grad_value.to(g.dtype) for g in ctx.grads)


class Regularizer(object):
    """alpha, beta, gamma: a number for every inverted field, or a dict keyed by module.NAMES (a missing name: 0).  prior: the fields
    at construction (cloned), or a tuple in module.NAMES order / a dict of tensors.  scale: mean |prior| of each field, or a number /
    tuple / dict.  weight: None or a non-negative (nz, nx) tensor.  dx, dz: the grid spacings of the module's parameter file.  A field
    of the module that is not a parameter is skipped."""

    def __init__(self, module, alpha=0.0, beta=0.0, gamma=0.0, eps=1e-3, prior=None, scale=None, weight=None, dx=None, dz=None):
        self.module = module
        self.names = tuple(module.NAMES)
        params = dict(module.named_parameters())
        self.active = tuple(n for n in self.names if n in params)
        if not self.active:
            raise ValueError("Regularizer: the module inverts for none of its fields")

        def per_field(x, default=None):
            if isinstance(x, dict):
                x = [x.get(n, default) for n in self.names]
            elif not isinstance(x, (tuple, list)):
                x = [x] * len(self.names)
            return {n: float(x[self.names.index(n)]) for n in self.active}
        self.alpha, self.beta, self.gamma = per_field(alpha, 0.0), per_field(beta, 0.0), per_field(gamma, 0.0)
        self.eps = float(eps)
        if prior is None:
            prior = {n: params[n] for n in self.active}
        elif not isinstance(prior, dict):
            prior = dict(zip(self.names, prior))
        self.prior = {n: prior[n].detach().clone().to(device=params[n].device, dtype=params[n].dtype).contiguous() for n in self.active}
        for n in self.active:
            if tuple(self.prior[n].shape) != tuple(params[n].shape) or params[n].dim() != 2:
                raise ValueError("Regularizer: prior of %s must have the field's shape (nz, nx)" % n)
        self.scale = {n: float(self.prior[n].abs().double().mean()) for n in self.active} if scale is None else per_field(scale)
        ref = params[self.active[0]]
        self.weight = None if weight is None else weight.detach().to(device=ref.device, dtype=ref.dtype).contiguous()
        if dx is None or dz is None:
            para = _utils.read_para(module.para_fname)
            dx, dz = (para["dx"] if dx is None else dx), (para["dz"] if dz is None else dz)
        self.dx, self.dz = float(dx), float(dz)
        ok = lambda x: x == x and x not in (float("inf"), float("-inf"))
        for n in self.active:
            if not all(ok(x) and x >= 0 for x in (self.alpha[n], self.beta[n], self.gamma[n])):
                raise ValueError("Regularizer: alpha, beta and gamma must be finite and non-negative")
            if not (ok(self.scale[n]) and self.scale[n] > 0):
                raise ValueError("Regularizer: the scale of %s must be positive (a zero prior needs scale=)" % n)
        if not (self.dx > 0 and self.dz > 0) or (any(self.gamma[n] > 0 for n in self.active) and not self.eps > 0):
            raise ValueError("Regularizer: dx, dz and (with a gamma) eps must be positive")
        if self.weight is not None and tuple(self.weight.shape) != tuple(ref.shape):
            raise ValueError("Regularizer: weight must have the fields' shape")

    # -- public ----------------------------------------------------------------------------------------------------------------------
    def __call__(self):
        """R at the module's current fields: a scalar tensor, differentiable with respect to the module's parameters."""
        return _RegFunction.apply(self, *[getattr(self.module, n) for n in self.active])

    def value_and_grad(self):
        """-> (R as a float64 scalar tensor on the fields' device, the gradient as a tuple in module.NAMES order with None for a field
        that is not inverted)."""
        value, grads = self._value_and_grad([getattr(self.module, n).detach() for n in self.active])
        by_name = dict(zip(self.active, grads))
        return value, tuple(by_name.get(n) for n in self.names)

    def hvp(self, v):
        """The exact Hessian of R at the module's current fields times v: a tuple in module.NAMES order (None: a field that is not
        perturbed) -> a tuple in that order, None where v has None or the field is not inverted (there is no coupling between fields)."""
        if len(v) != len(self.names):
            raise ValueError("hvp: v must have one entry per field of the module (None: not perturbed)")
        fields, vs = [], []
        for n, t in zip(self.names, v):
            if n not in self.active or t is None:
                fields.append(None), vs.append(None)
                continue
            f = getattr(self.module, n).detach()
            if not torch.is_tensor(t) or tuple(t.shape) != tuple(f.shape):
                raise ValueError("hvp: the entry of %s must be a tensor of shape %s (or None)" % (n, tuple(f.shape)))
            fields.append(f), vs.append(t.detach().to(device=f.device, dtype=f.dtype))
        names = [n for n, t in zip(self.names, vs) if t is not None]
        if not names:
            return tuple(None for _ in self.names)
        f_on, v_on = [t for t in fields if t is not None], [t for t in vs if t is not None]
        if self._fusable(f_on):
            out = self._launch(names, f_on, v_on)[1]
        else:
            out = [self._torch_hvp(n, f, t) for n, f, t in zip(names, f_on, v_on)]
        by_name = dict(zip(names, out))
        return tuple(by_name.get(n) for n in self.names)

    # -- the two paths ---------------------------------------------------------------------------------------------------------------
    def _fusable(self, fields):
        dev = fields[0].device
        return (USE_FUSED and all(t.is_cuda and t.dtype == torch.float32 and t.device == dev and t.dim() == 2
                                  and t.shape == fields[0].shape for t in fields)
                and all(p.device == dev and p.dtype == torch.float32 for p in self.prior.values())
                and (self.weight is None or (self.weight.device == dev and self.weight.dtype == torch.float32)))

    def _value_and_grad(self, fields):
        if self._fusable(fields):
            return self._launch(list(self.active), fields, None)
        parts = [self._torch_value_grad(n, f) for n, f in zip(self.active, fields)]
        return sum(p[0] for p in parts), [p[1] for p in parts]

    def _launch(self, names, fields, v):
        """One call of sepfwi_regularizer (v None: -> (value, gradients)) or sepfwi_regularizer_hvp (-> (None, products)) for the
        fields `names` (a module has three)."""
        L = _native.lib()
        dev = fields[0].device
        nz, nx = fields[0].shape
        triple, stream = _native.triple, _native.stream_arg(dev)
        floats = lambda d, fill=0.0: (C.c_float * 3)(*([d[n] for n in names] + [fill] * (3 - len(names))))
        f = [t.contiguous() for t in fields]
        outs = [torch.empty_like(t) for t in f]
        args = [int(nz), int(nx), self.dx, self.dz, triple(f), triple([self.prior[n] for n in names]), _native.ptr(self.weight),
                floats(self.alpha), floats(self.beta), floats(self.gamma), floats(self.scale, 1.0), self.eps]
        if v is None:
            value = torch.empty((), dtype=torch.float64, device=dev)      # the sum kernel writes it: nothing waits for it here
            _native.check(L.sepfwi_regularizer(*args, _native.ptr(value), triple(outs), stream))
            return value, outs
        vv = [t.contiguous() for t in v]
        _native.check(L.sepfwi_regularizer_hvp(*args, triple(vv), triple(outs), stream))
        return None, outs

    def _consts(self, n, like):
        s = self.scale[n]
        w = 1.0 if self.weight is None else self.weight.to(like.dtype)
        return w, 1.0 / (s * self.dx), 1.0 / (s * self.dz), self.alpha[n] / (s * s), self.beta[n], self.gamma[n]

    def _torch_value_grad(self, n, p):
        """the operation list of csrc/regularizer.hip in torch, in p's dtype; the cell energies are summed in float64"""
        w, rx, rz, a2, beta, gamma = self._consts(n, p)
        gx, gz = _diff(p, rx, rz)
        n2 = gx * gx + gz * gz
        e, t0 = torch.zeros_like(p), torch.zeros_like(p)
        if a2 > 0:
            d = p - self.prior[n].to(p.dtype)
            t0 = (w * a2) * d
            e = (0.5 * a2) * (d * d)
        c = torch.full_like(p, beta)
        et = (0.5 * beta) * n2
        if gamma > 0:
            phi = torch.sqrt(n2 + self.eps * self.eps)
            c = c + gamma / phi
            et = et + gamma * (n2 / (phi + self.eps))
        c = w * c
        return (w * (e + et)).double().sum(), _gather(t0, c * gx, c * gz, rx, rz)

    def _torch_hvp(self, n, p, v):
        w, rx, rz, a2, beta, gamma = self._consts(n, p)
        qx, qz = _diff(v, rx, rz)
        tx, tz = beta * qx, beta * qz
        if gamma > 0:
            gx, gz = _diff(p, rx, rz)
            iphi = 1.0 / torch.sqrt((gx * gx + gz * gz) + self.eps * self.eps)
            iphi3, c, e2 = (iphi * iphi) * iphi, gx * qz - gz * qx, self.eps * self.eps
            tx = tx + gamma * ((e2 * qx - gz * c) * iphi3)      # q / phi - g (g.q) / phi^3 without its cancellation (csrc/regularizer.hip)
            tz = tz + gamma * ((e2 * qz + gx * c) * iphi3)
        t0 = (w * a2) * v if a2 > 0 else torch.zeros_like(v)
        return _gather(t0, w * tx, w * tz, rx, rz)
