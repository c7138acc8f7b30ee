"""SciPy <-> torch glue for L-BFGS-B (reference: obj_wrapper.py:10-97): flat float64 vector in, (loss,
flat float64 gradient) out, with a one-entry cache so fun(x) and jac(x) share one propagation."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch
from scipy import optimize


class PyTorchObjective(object):
    """fun / jac / hessp of `loss` over the parameters of the module `obj` as flat float64 vectors.

    smoother=  a sepfwi.smooth.Smoother S (None: the unknowns are the parameters themselves, every bit as without the argument): the
               unknown is y with x0 = 0, and the module's parameter k is loaded as p_ref_k + s_k S y_k, p_ref the parameters at
               construction.  jac packs s_k S^T grad_k and hessp returns s S^T H (s S p) with the regulariser's product inside: the
               gradient and the (Gauss-Newton) Hessian of the same loss in y, exactly, because S^T is the exact transpose.
    scales=    s_k: a number, a tuple in named_parameters() order or a dict by name; None: mean |p_ref_k| (1 where that is 0).
    With a smoother `bounds` is None: a box p_lo <= p <= p_hi has no separable image under S -- every y_k moves a neighbourhood of
    cells -- so the per-variable bounds that L-BFGS-B takes cannot express it."""

    def __init__(self, obj, loss, shot_ids=None, exact=True, regularizer=None, smoother=None, scales=None):
        self.obj = obj      # nn.Module holding the parameters (and .Bounds)
        self.loss = loss    # callable -> scalar tensor
        self.shot_ids = shot_ids   # for hessp: the shots of obj.gauss_newton (None: no hessp)
        self.exact = exact         # ... and its adjoint (True: symmetric and non-negative, what trust-ncg / Newton-CG assume)
        self.regularizer = regularizer   # for hessp: a sepfwi.regularize.Regularizer whose term `loss` adds (None: no model term)
        params = OrderedDict(obj.named_parameters())
        self.param_shapes = OrderedDict((n, tuple(p.shape)) for n, p in params.items())
        self.x0 = np.concatenate([p.data.cpu().numpy().ravel() for p in params.values()]).astype(np.float64)
        self.bounds = self.pack_bounds() if getattr(obj, "Bounds", {}) != {} else None
        self.smoother = smoother
        if smoother is not None:
            self.p_ref = OrderedDict((n, p.detach().clone()) for n, p in params.items())
            if scales is None:
                scales = [float(p.abs().double().mean()) or 1.0 for p in self.p_ref.values()]
            elif isinstance(scales, dict):
                scales = [float(scales[n]) for n in params]
            elif not isinstance(scales, (tuple, list)):
                scales = [float(scales)] * len(params)
            if len(scales) != len(params) or not all(np.isfinite(x) and x > 0 for x in scales):
                raise ValueError("scales must be one finite positive number per parameter")
            self.scales = OrderedDict(zip(params, (float(x) for x in scales)))
            self.x0 = np.zeros_like(self.x0)
            self.bounds = None

    def smoothed(self, by_name, transpose=False):
        """{name: tensor} -> {name: s_k S tensor} (or s_k S^T tensor) on the parameters' device and dtype"""
        names = tuple(getattr(self.obj, "NAMES", ()))
        if not all(n in names for n in self.p_ref):
            names = tuple(self.p_ref)
        ts = tuple(by_name[n].to(device=self.p_ref[n].device, dtype=self.p_ref[n].dtype) if n in by_name else None for n in names)
        out = self.smoother.apply_t(ts) if transpose else self.smoother.apply(ts)
        return OrderedDict((n, self.scales[n] * t) for n, t in zip(names, out) if t is not None)

    def unpack_parameters(self, x):
        out, i = OrderedDict(), 0
        for n, shp in self.param_shapes.items():
            k = int(np.prod(shp))
            out[n] = torch.from_numpy(np.asarray(x[i:i + k]).reshape(shp))
            i += k
        return out

    def pack_grads(self):
        if self.smoother is not None:
            g = self.smoothed(OrderedDict((n, p.grad.data) for n, p in self.obj.named_parameters()), transpose=True)
            return np.concatenate([g[n].cpu().numpy().ravel() for n in self.param_shapes]).astype(np.float64)
        return np.concatenate([p.grad.data.cpu().numpy().ravel() for p in self.obj.parameters()]).astype(np.float64)

    def pack_bounds(self):
        lo = [np.asarray(self.obj.Bounds[n][0]).ravel() for n in self.param_shapes]
        hi = [np.asarray(self.obj.Bounds[n][1]).ravel() for n in self.param_shapes]
        return optimize.Bounds(np.concatenate(lo).astype(np.float64), np.concatenate(hi).astype(np.float64))

    def is_new(self, x):
        if not hasattr(self, "cached_x"):
            return True
        return np.abs(np.array(x) - np.array(self.cached_x)).max() > 1e-8

    def load(self, x):
        state = self.unpack_parameters(x)
        if self.smoother is not None:
            state = OrderedDict((n, self.p_ref[n] + t) for n, t in self.smoothed(state).items())
        for name, buf in self.obj.named_buffers():
            state[name] = buf
        self.obj.load_state_dict(state)

    def cache(self, x):
        self.load(x)
        self.cached_x = x
        self.obj.zero_grad()
        val = self.loss()
        self.f = val.item()
        val.backward()
        self.jac = self.pack_grads()

    def fun(self, x):
        if self.is_new(x):
            self.cache(x)
        return self.f

    def jac(self, x):
        if self.is_new(x):
            self.cache(x)
        return self.jac

    def hessp(self, x, p):
        """The Gauss-Newton Hessian at x times p, flat float64 in and out -- what `optimize.minimize(fun, x0, jac=, hessp=,
        method="trust-ncg")` (or "Newton-CG") takes; an extension without a counterpart in the reference.  p is scattered over the
        module's parameters in named_parameters() order (a field of the module that is not a parameter gets None), the product is
        obj.gauss_newton(v, shot_ids, exact=exact), and the entries of the parameters are packed as `jac` packs the gradient.
        Under a parameter file with if_envelope_misfit the product is the envelope misfit's own Gauss-Newton Hessian (include/sepfwi.h,
        sepfwi_born): nothing changes here.  Under if_w2_misfit the library refuses the product (SepFwiError, SEPFWI_EINVAL: the transport
        misfit has no Gauss-Newton form here) and the error surfaces as it stands; L-BFGS-B needs `fun` / `jac` alone.  Under robust_misfit the
        product is the IRLS Gauss-Newton form J^T C^T Z W Z C J (W the Huber / Cauchy weight at the current model): positive semi-definite, nothing changes here.  With `regularizer=` its exact Hessian-vector product regularizer.hvp(v) is added, field by
        field, to the Gauss-Newton product: the Hessian of the model term that `loss` carries as `+ regularizer()`.  With `smoother=`
        x and p are in the smoothed variables y: the product is s S^T H (s S p), H the sum above at the model p_ref + s S x."""
        if self.shot_ids is None:
            raise ValueError("hessp needs the shots of the Gauss-Newton product: PyTorchObjective(obj, loss, shot_ids=...)")
        if not hasattr(self.obj, "gauss_newton"):
            raise ValueError("hessp needs a module with a gauss_newton(v, Shot_ids, exact=) method")
        if self.is_new(x):
            self.load(x)
            self.__dict__.pop("cached_x", None)      # the module has left the cached point: the next fun / jac evaluates again
        params = OrderedDict(self.obj.named_parameters())
        fields = tuple(getattr(self.obj, "NAMES", tuple(params)))
        chunks = self.unpack_parameters(np.asarray(p, dtype=np.float64))
        if self.smoother is not None:
            chunks = self.smoothed(chunks)
        v = tuple(chunks[n].to(device=params[n].device, dtype=params[n].dtype) if n in params else None for n in fields)
        hv = self.obj.gauss_newton(v, self.shot_ids, exact=self.exact)
        if self.regularizer is not None:
            hv = tuple(h if r is None else h + r.to(h.dtype) for h, r in zip(hv, self.regularizer.hvp(v)))
        if self.smoother is not None:
            back = self.smoothed(OrderedDict((n, hv[fields.index(n)].detach()) for n in params), transpose=True)
            return np.concatenate([back[n].cpu().numpy().ravel() for n in params]).astype(np.float64)
        return np.concatenate([hv[fields.index(n)].detach().cpu().numpy().ravel() for n in params]).astype(np.float64)


_SETULB_SIGNATURE = "setulb(m,x,l,u,nbd,f,g,factr,pgtol,wa,iwa,task,lsave,isave,dsave,maxls,ln_task)"


def minimize_lbfgsb(fun, x0, jac, bounds=None, callback=None, maxiter=15000, maxcor=10, ftol=2.2204460492503131e-09, gtol=1e-5,
                    maxfun=15000, maxls=20, scale=None):
    """`optimize.minimize(fun, x0, method="L-BFGS-B", jac=jac, bounds=bounds, callback=callback, options={...})` -- what the
    reference's experiment scripts call (Main-001-FWI-Anomaly-Vp-Vs-Den.py:157-168) -- with the same compiled routine
    (`scipy.optimize._lbfgsb.setulb`) driven directly, so the iterates are the same bit for bit, but without SciPy's
    per-element Python loops over the bounds: on the 6 M unknowns of a 2000 x 1000 model those cost 10-20 s per minimize() call
    (new-style -> old-style -> new-style conversions and a dict look-up per variable), the one serial term of a multi-GPU
    inversion that does not shrink with the number of GPUs.  Here the bound codes are three vectorised
    numpy expressions.  `bounds`: an `optimize.Bounds` or None.  Falls back to `optimize.minimize` when there are no bounds
    (nothing to save) or when the installed SciPy's private routine does not have the signature this driver was written for.
    `scale`: None, or a positive vector s (a diagonal preconditioner, e.g. (pseudo-Hessian)^(-1/2)): the routine optimises
    y = x / s -- function and gradient are evaluated at x = s y with g_y = s g_x, the bounds are divided by s -- while the callback
    and the result (x, jac) are in x.  With None the iterates are bit for bit those without the argument."""
    if scale is not None:
        s = np.asarray(scale, dtype=np.float64).ravel()
        x0 = np.asarray(x0, dtype=np.float64).ravel()
        if s.size != x0.size or not (np.isfinite(s).all() and (s > 0).all()):
            raise ValueError("scale must be a finite positive vector of the size of x0")
        lb = ub = None
        if bounds is not None:
            lb = np.broadcast_to(np.asarray(bounds.lb, dtype=np.float64), x0.shape)
            ub = np.broadcast_to(np.asarray(bounds.ub, dtype=np.float64), x0.shape)
        to_x = (lambda y: s * y) if bounds is None else (lambda y: np.clip(s * y, lb, ub))   # (s (lb / s) may miss lb by an ulp)
        res = minimize_lbfgsb(lambda y: fun(to_x(y)), x0 / s, lambda y: s * np.asarray(jac(to_x(y)), dtype=np.float64),
                              bounds=None if bounds is None else optimize.Bounds(lb / s, ub / s),
                              callback=None if callback is None else (lambda y: callback(to_x(y))), maxiter=maxiter, maxcor=maxcor,
                              ftol=ftol, gtol=gtol, maxfun=maxfun, maxls=maxls)
        res.x = to_x(res.x)
        res.jac = np.asarray(res.jac, dtype=np.float64) / s
        if "hess_inv" in res:
            del res["hess_inv"]   # it is that of the scaled problem
        return res
    options = dict(maxiter=maxiter, maxcor=maxcor, ftol=ftol, gtol=gtol, maxfun=maxfun, maxls=maxls)
    try:
        from scipy.optimize import _lbfgsb
        fast = bounds is not None and (_lbfgsb.setulb.__doc__ or "").strip().startswith(_SETULB_SIGNATURE)
    except ImportError:
        fast = False
    if not fast:
        return optimize.minimize(fun, x0, method="L-BFGS-B", jac=jac, bounds=bounds, callback=callback, options=options)
    x = np.array(x0, dtype=np.float64).ravel()
    n, m = x.size, int(maxcor)
    lb = np.broadcast_to(np.asarray(bounds.lb, dtype=np.float64), (n,))
    ub = np.broadcast_to(np.asarray(bounds.ub, dtype=np.float64), (n,))
    if (lb > ub).any():
        raise ValueError("LBFGSB - one of the lower bounds is greater than an upper bound.")
    if not maxls > 0:
        raise ValueError("maxls must be positive.")
    x = np.clip(x, lb, ub)
    has_lo, has_hi = np.isfinite(lb), np.isfinite(ub)
    nbd = np.where(has_lo & has_hi, 2, np.where(has_lo, 1, np.where(has_hi, 3, 0))).astype(np.int32)   # setulb's bound codes
    low_bnd, upper_bnd = np.where(has_lo, lb, 0.0), np.where(has_hi, ub, 0.0)
    factr = ftol / np.finfo(float).eps

    state = {"x": None, "f": None, "g": None, "nfev": 0}

    def fun_and_grad(xk):       # one evaluation per distinct point, as SciPy's ScalarFunction counts them
        if state["x"] is None or not np.array_equal(xk, state["x"]):
            state["x"] = np.copy(xk)
            state["f"] = float(fun(np.copy(xk)))
            state["g"] = np.asarray(jac(np.copy(xk)), dtype=np.float64)
            state["nfev"] += 1
        return state["f"], state["g"]

    fun_and_grad(x)             # SciPy evaluates at x0 while it builds its ScalarFunction
    f = np.array(0.0, dtype=np.float64)
    g = np.zeros(n, dtype=np.float64)
    wa = np.zeros(2 * m * n + 5 * n + 11 * m * m + 8 * m, np.float64)
    iwa = np.zeros(3 * n, dtype=np.int32)
    task, ln_task = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    lsave, isave, dsave = np.zeros(4, dtype=np.int32), np.zeros(44, dtype=np.int32), np.zeros(29, dtype=np.float64)
    nit = 0
    while True:
        g = np.asarray(g, dtype=np.float64)
        _lbfgsb.setulb(m, x, low_bnd, upper_bnd, nbd, f, g, factr, gtol, wa, iwa, task, lsave, isave, dsave, maxls, ln_task)
        if task[0] == 3:        # FG: the routine wants f and g at x
            f, g = fun_and_grad(x)
        elif task[0] == 1:      # NEW_X: an iteration is complete
            nit += 1
            halt = False
            if callback is not None:
                try:
                    callback(np.copy(x))
                except StopIteration:
                    halt = True
            if halt:
                task[0], task[1] = 5, 505
            if nit >= maxiter:
                task[0], task[1] = 5, 504
            elif state["nfev"] > maxfun:
                task[0], task[1] = 5, 502
        else:
            break
    from scipy.optimize._lbfgsb_py import status_messages, task_messages
    status = 0 if task[0] == 4 else (1 if (state["nfev"] > maxfun or nit >= maxiter) else 2)
    n_corrs = min(int(isave[30]), m)
    s, y = wa[0:m * n].reshape(m, n), wa[m * n:2 * m * n].reshape(m, n)
    return optimize.OptimizeResult(fun=float(f), jac=g, nfev=state["nfev"], njev=state["nfev"], nit=nit, status=status,
                                   message=status_messages[task[0]] + ": " + task_messages[task[1]], x=x, success=(status == 0),
                                   hess_inv=optimize.LbfgsInvHessProduct(s[:n_corrs], y[:n_corrs]))


def gauss_newton_cg(hessvec, grad, damping=0.0, diag=None, maxiter=10, rtol=1e-2, callback=None, precond=None):
    """Matrix-free (preconditioned) conjugate gradients for the Gauss-Newton step:  (H + damping D) p = -g.

    hessvec   callable: a tuple of tensors v -> the tuple H v (fwi_ops.gauss_newton at a fixed model; an extension without a
              counterpart in the reference).  The parameter file decides which misfit's product that is: J^T W J, J^T C^T Z C J under
              if_win / filter, J^T C^T D^T Z D C J under if_envelope_misfit, the IRLS form J^T C^T Z W Z C J under robust_misfit (under if_w2_misfit the library refuses it) -- symmetric and non-negative with exact=True in every case,
              which is all this solver needs.  A model term composes as `lambda v: add(H(v), reg.hvp(v))` (sepfwi.regularize)
    grad      the gradient g, a tuple of tensors shaped like v
    diag      optional tuple of non-negative tensors, e.g. the diagonal pseudo-Hessian: D in the damping term AND the Jacobi
              preconditioner M = D (zero entries -- outside the illuminated region -- are floored at 1e-12 max D); None: D = M = I
    precond   optional callable: a tuple of tensors r -> the tuple M^-1 r, M^-1 symmetric and non-negative, e.g.
              sepfwi.smooth.Smoother.preconditioner(diag) = D^-1/2 S S^T D^-1/2.  It REPLACES the Jacobi preconditioner; diag keeps its
              role in the damping term.  None: every bit as without the argument
    maxiter   fixed cap on the products; rtol: stop once |r| <= rtol |g| in the preconditioned norm sqrt(r^T M^-1 r)
    -> (p, history): the step as a list of tensors and the relative residual before every iteration and after the last one
    (history[0] = 1).  An iteration that meets non-positive curvature (the reference's adjoint is not exact) stops the solve with the
    step found so far (the scaled steepest-descent direction if it is the first)."""
    g = [t.detach() for t in grad]
    dot = lambda a, b: float(sum((x.double() * y.double()).sum() for x, y in zip(a, b)))
    if diag is None:
        minv = None
        D = None
    else:
        D = [d.detach().clamp_min(0) for d in diag]
        minv = [1.0 / d.clamp_min(1e-12 * float(d.max()) if float(d.max()) > 0 else 1.0) for d in D]
    prec = (lambda r: [t.clone() for t in r]) if minv is None else (lambda r: [a * b for a, b in zip(minv, r)])
    if precond is not None:
        prec = lambda r: [t.detach() for t in precond(tuple(r))]

    def A(v):
        hv = [t.detach() for t in hessvec(tuple(v))]
        if damping:
            hv = [h + damping * (x if D is None else D[k] * x) for k, (h, x) in enumerate(zip(hv, v))]
        return hv

    p = [torch.zeros_like(t) for t in g]
    r = [-t for t in g]
    z = prec(r)
    d = [t.clone() for t in z]
    rz = dot(r, z)
    rz0 = rz
    hist = [1.0]
    if not rz0 > 0:
        return p, hist
    for it in range(int(maxiter)):
        Ad = A(d)
        curv = dot(d, Ad)
        if not curv > 0:
            if it == 0:
                p = [t.clone() for t in d]
            break
        alpha = rz / curv
        p = [a + alpha * b for a, b in zip(p, d)]
        r = [a - alpha * b for a, b in zip(r, Ad)]
        z = prec(r)
        rz_new = dot(r, z)
        hist.append(float(np.sqrt(max(rz_new, 0.0) / rz0)))
        if callback is not None:
            callback(it + 1, hist[-1])
        if hist[-1] <= rtol:
            break
        d = [a + (rz_new / rz) * b for a, b in zip(z, d)]
        rz = rz_new
    return p, hist
