"""Operator boundary: same surface as the reference's JIT-built extension `fwi_ops` and its autograd
Function (DAS_Waveform_Inversion/Ops/FWI/FWI_ops.py:15-63, Src/Torch_Fwi.cpp:12-142), backed by
libsepfwi.so through ctypes.  No CPU fallback exists.

Multi-GPU:
  * under torch.distributed (one process per GPU, launched by torchrun) every rank works on its
    contiguous block of Shot_ids and ONE all-reduce (RCCL on GPUs, gloo on CPU tests) sums the fused
    buffer [gLambda | gMu | gDen | misfit]  -- see dist.py;
  * without torch.distributed, `ngpu` > 1 drives that many devices from one process with one host
    thread each, the reference's own model (OpenMP, Src/Torch_Fwi.cpp:71-95).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _native
from . import dist as _dist
from . import utils as _utils


def split_shots(group_size: int, ngpu: int):
    """Start offsets of the per-GPU shot blocks: int(float32 linspace(0, n, ngpu+1))
    (Src/Torch_Fwi.cpp:59-60,78-80)."""
    if ngpu > group_size:
        raise RuntimeError("The number of GPUs should be smaller than the number of shots!")  # Torch_Fwi.cpp:49-52
    return torch.linspace(0, group_size, ngpu + 1, dtype=torch.float32).to(torch.int32).tolist()


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if not torch.is_tensor(t):
        raise TypeError("%s must be a torch tensor" % name)
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (the reference reads data_ptr<float>(), Torch_Fwi.cpp:55-58)" % name)
    return t.detach().contiguous()


# An armed call is arm -> run -> collect -> disarm on ONE session: threads that share a session (single-process ngpu > 1 with the
# device pinned) take turns, or one would collect the other's result.
_PH_LOCKS = {}
_PH_GUARD = threading.Lock()


def _ph_lock(para_fname, gpu_id):
    with _PH_GUARD:
        return _PH_LOCKS.setdefault((str(para_fname), int(gpu_id)), threading.Lock())


def _para_dims(para_fname):
    """(nz, nx, nSteps) of the one-line parameter JSON (fwi_utils.py:46-83), cached (utils.read_para).  The reference passes raw
    data_ptr<float>()s with no size anywhere (Src/Torch_Fwi.cpp:55-58); here a tensor of the wrong shape is an error
    before the library reads or writes past it."""
    try:
        p = _utils.read_para(para_fname)
        return int(p["nz"]), int(p["nx"]), int(p["nSteps"])
    except (OSError, ValueError, KeyError, TypeError):
        return None          # the library reports the missing (SEPFWI_EIO) or malformed (SEPFWI_EJSON) file


def _shot_ids(shot_ids):
    """Shot_ids as the library reads them: a tensor on any device, a list or an array -> a contiguous 1-D int32 numpy array"""
    return np.ascontiguousarray(np.asarray(shot_ids.cpu() if torch.is_tensor(shot_ids) else shot_ids, dtype=np.int32)).reshape(-1)


def _checked(Lambda, Mu, Den, Stf, shot_ids, para_fname, what, v=(), need_dims=True):
    """What _cufd, _born and _adjoint_exact do to their arguments before anything is allocated: float32 contiguous tensors, one
    shape and one device for the model (and the perturbation v), Stf and Shot_ids against the parameter file.
    -> (Lambda, Mu, Den, Stf, v, ids, nSteps); nSteps is None where the parameter file cannot be read and need_dims is false (the
    library then reports the file)."""
    Lambda, Mu, Den, Stf = _f32c(Lambda, "Lambda"), _f32c(Mu, "Mu"), _f32c(Den, "Den"), _f32c(Stf, "Stf")
    v = [_f32c(t, n) for t, n in zip(v, ("dLambda", "dMu", "dDen"))]
    names = "Lambda, Mu, Den, dLambda, dMu, dDen" if v else "Lambda, Mu, Den"
    if Lambda.dim() != 2 or any(t.shape != Lambda.shape for t in [Mu, Den] + v):
        raise ValueError(names + " must be 2-D tensors of one shape (nz_pad, nx_pad)")
    if any(t.device != Lambda.device for t in [Mu, Den] + v):
        raise ValueError(names + " must live on one device")
    ids = _shot_ids(shot_ids)
    dims = _para_dims(para_fname)
    if dims is None:
        if need_dims:
            raise ValueError("cannot read nz, nx, nSteps from the parameter file %r" % (para_fname,))
        return Lambda, Mu, Den, Stf, v, ids, None
    nz, nx, nSteps = dims
    if tuple(Lambda.shape) != (nz, nx):
        raise ValueError("%s %s but the parameter file says (nz, nx) = (%d, %d)" % (what, tuple(Lambda.shape), nz, nx))
    if Stf.dim() != 2 or Stf.shape[1] != nSteps:
        raise ValueError("Stf must be (nSrc, nSteps = %d), got %s" % (nSteps, tuple(Stf.shape)))
    if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= Stf.shape[0]):
        raise ValueError("Shot_ids must index rows of Stf (0..%d), got %d..%d" % (Stf.shape[0] - 1, int(ids.min()), int(ids.max())))
    return Lambda, Mu, Den, Stf, v, ids, nSteps


def _gdev(Lambda, gpu_id):
    """Where a call's outputs are allocated, so that the session writes them in place: on ITS GPU when the model lives on a GPU (also
    another one: single-process ngpu > 1), on the host for the reference's CPU tensors."""
    return torch.device("cuda", gpu_id) if Lambda.is_cuda else torch.device("cpu")


def _stream_for(t, dev):
    """The stream argument of a call that reads or writes t on the session of HIP device dev: torch's current stream when t lives
    there; else None (the legacy default stream: the library orders itself behind it), after t's own GPU, if any, has finished."""
    if t.is_cuda and t.device.index == dev:
        return _native.stream_arg(t.device)
    if t.is_cuda:
        torch.cuda.synchronize(t.device)   # produced on another GPU: finished before it is staged
    return None


def _stream_or_sync(Lambda, Stf, gpu_id, sync_current=False):
    """The stream argument of a call (_stream_for the model), after everything it reads has been queued."""
    if sync_current and Lambda.is_cuda:         # (on another GPU than the session's, _stream_for waits for the whole device anyway)
        torch.cuda.current_stream(Lambda.device).synchronize()
    stream = _stream_for(Lambda, gpu_id)
    if Stf.is_cuda:
        torch.cuda.synchronize(Stf.device)      # read with a blocking copy inside the library
    return stream


def _nrec_per_shot(para_fname, ids):
    """Channels of every shot of ids, from the survey file the parameter file names (cached: utils.read_survey_channels)."""
    channels = _utils.read_survey_channels(para_fname)
    for i in ids:
        if "shot%d" % int(i) not in channels:
            raise ValueError("shot id %d is not in the survey file" % int(i))
    return [channels["shot%d" % int(i)] for i in ids]


def _local_rows(dStf, Stf, ids, gdev):
    """A source perturbation in Stf's shape (nSrc, nSteps) -> its rows of Shot_ids, the library's local layout (row i: ids[i])."""
    dStf = _f32c(dStf, "dStf")
    if dStf.shape != Stf.shape:
        raise ValueError("dStf must have the shape of Stf %s, got %s" % (tuple(Stf.shape), tuple(dStf.shape)))
    return dStf[torch.as_tensor(ids, dtype=torch.long, device=dStf.device)].to(gdev).contiguous()


def _global_rows(g_loc, Stf, ids):
    """The library's (len(ids), nSteps) source block -> Stf's shape on the host (as gStf of backward): rows of Shot_ids scattered (a shot
    named twice adds up), all other rows zero."""
    out = torch.zeros(tuple(Stf.shape), dtype=torch.float32)
    out.index_add_(0, torch.as_tensor(ids, dtype=torch.long), g_loc.cpu())
    return out


class _FwiOps:
    """Module object: fwi_ops.forward / backward / obscalc."""

    def __init__(self):
        self.device_override = None   # bench/tests may pin the HIP device index

    # -- one cufd call on one device ------------------------------------------------------
    def _cufd(self, calc_id, gpu_id, Lambda, Mu, Den, Stf, shot_ids, para_fname, out_device=None, pseudo_hessian=0):
        """-> (misfit, gL, gM, gD, gS); with pseudo_hessian = k > 0 (calc_id 0 / 1) the session is armed with every = k for this call
        alone and a sixth entry follows: the fused (3, nz, nx) tensor [hLambda | hMu | hDen] of the call's shots."""
        L = _native.lib()
        k = int(pseudo_hessian)
        if k < 0:
            raise ValueError("pseudo_hessian must be >= 0 (0: off, k: accumulate on every k-th forward step)")
        if k > 0 and calc_id not in (0, 1):
            raise ValueError("pseudo_hessian needs a misfit or gradient call")
        Lambda, Mu, Den, Stf, _, ids, _ = _checked(Lambda, Mu, Den, Stf, shot_ids, para_fname, "Lambda/Mu/Den are", need_dims=False)
        gpu_id = int(gpu_id)
        dev = out_device if out_device is not None else Lambda.device
        gdev = _gdev(Lambda, gpu_id)
        # the loss lives where the model lives (the reference: CPU tensors throughout, torch::zeros(1)); calc_id 1 below makes it the
        # last element of the gradient buffer
        misfit = torch.zeros(1, dtype=torch.float32, device=gdev if calc_id == 0 else "cpu")
        gL = gM = gD = gS = None
        if calc_id == 1:
            # ONE buffer [gLambda | gMu | gDen | misfit]: the session writes all four in place, and under torch.distributed
            # this very buffer is what the single all-reduce sums (dist.allreduce_gradients) -- no staging, misfit stays in HBM
            n = Lambda.numel()
            fused = torch.zeros(3 * n + 1, dtype=torch.float32, device=gdev)
            gL, gM, gD = (fused[k * n:(k + 1) * n].view(Lambda.shape) for k in range(3))
            misfit = fused[3 * n:3 * n + 1]
            gS = torch.zeros((int(ids.size), Stf.shape[1]), dtype=torch.float32)
        stream = _stream_or_sync(Lambda, Stf, gpu_id)
        fn = _native.path_arg(para_fname)
        H = None
        with (_ph_lock(para_fname, gpu_id) if k > 0 else contextlib.nullcontext()):
            if k > 0:
                _native.check(L.sepfwi_pseudo_hessian_arm(fn, gpu_id, k))
            try:
                rc = L.sepfwi_cufd_stream(_native.ptr(misfit), _native.ptr(gL), _native.ptr(gM), _native.ptr(gD), _native.ptr(gS), _native.ptr(Lambda), _native.ptr(Mu), _native.ptr(Den),
                                          _native.ptr(Stf), int(calc_id), gpu_id, int(ids.size), _native.ids_arg(ids), fn, stream, 0)
                _native.check(rc)
                if k > 0:   # ONE buffer [hLambda | hMu | hDen], the unit of the all-reduce under torch.distributed
                    H = torch.empty((3,) + tuple(Lambda.shape), dtype=torch.float32, device=gdev)
                    _native.check(L.sepfwi_get_pseudo_hessian(fn, gpu_id, _native.ptr(H[0]), _native.ptr(H[1]), _native.ptr(H[2])))
            finally:
                if k > 0:
                    L.sepfwi_pseudo_hessian_arm(fn, gpu_id, 0)   # disarm, also on error
        if H is not None and H.device != dev:
            H = H.to(dev)
        if calc_id == 1 and gL.device != dev:   # single-process ngpu > 1: every block's results return to the model's device
            gL, gM, gD, misfit = gL.to(dev), gM.to(dev), gD.to(dev), misfit.to(dev)
        elif calc_id == 0 and misfit.device != dev:   # forward(): the loss follows the model too, whatever gpu_id computed it
            misfit = misfit.to(dev)
        if k > 0:
            return misfit, gL, gM, gD, gS, H
        return misfit, gL, gM, gD, gS

    def _device_for(self, t: torch.Tensor, i: int, ngpu: int = 1) -> int:
        """HIP device of shot block `i` of `ngpu`: the pinned one (bench, tests); the tensors' own device for a single block or a
        rank of a torch.distributed job; LOCAL_RANK for a rank that holds the reference's CPU tensors; device i otherwise (the
        reference's omp thread i <-> GPU i, Src/Torch_Fwi.cpp:71-95)."""
        if self.device_override is not None:
            return int(self.device_override)
        if t.is_cuda and (ngpu == 1 or _dist.active()):
            return t.device.index or 0      # the tensors' own device, also under per-rank device masking (every rank sees one GPU)
        if _dist.active():
            return _dist.local_device_index()
        return i

    def _session_dev(self, gpu_id) -> int:
        """HIP device of the session an entry point with a `gpu_id` argument addresses: the pinned one, else gpu_id.  (stats and
        loop_status read gpu_id literally: bench.py passes them the device itself.)"""
        return int(gpu_id) if self.device_override is None else int(self.device_override)

    def _split_cufd(self, calc_id, Lambda, Mu, Den, Stf, ngpu, Shot_ids, para_fname, **kw):
        """_cufd over the shot split -> the list of its results: this rank's block under torch.distributed, one call for ngpu == 1,
        else one block and one host thread per GPU, every block's results on the model's device."""
        ids = _shot_ids(Shot_ids)
        if _dist.active():
            lo, hi = _dist.my_block(int(ids.size))
            return [self._cufd(calc_id, self._device_for(Lambda, 0), Lambda, Mu, Den, Stf, ids[lo:hi], para_fname, **kw)]
        ngpu = int(ngpu)
        bars = split_shots(int(ids.size), ngpu)
        if ngpu == 1:
            return [self._cufd(calc_id, self._device_for(Lambda, 0), Lambda, Mu, Den, Stf, ids, para_fname, **kw)]
        with ThreadPoolExecutor(max_workers=ngpu) as ex:   # one host thread per GPU, ctypes drops the GIL
            futs = [ex.submit(self._cufd, calc_id, self._device_for(Lambda, i, ngpu), Lambda, Mu, Den, Stf,
                              ids[bars[i]:bars[i + 1]], para_fname, Lambda.device, **kw) for i in range(ngpu)]
            return [f.result() for f in futs]

    # -- reference surface -------------------------------------------------------------------
    def backward(self, Lambda, Mu, Den, Stf, ngpu, Shot_ids, para_fname, *, pseudo_hessian=0, exact_adjoint=False, source_gradient=False):
        """-> [misfit(1,), gLambda, gMu, gDen, gStf]   (fwi_backward, Src/Torch_Fwi.cpp:38-104).
        Extension `exact_adjoint=True` (include/sepfwi.h, sepfwi_adjoint_exact): the same list, the gradients being the exact ones of
        the misfit on Omega (0 outside) and gStf ZEROS unless `source_gradient=True`: then gStf is the exact d misfit / d Stf
        (sepfwi_adjoint_exact_src), in Stf's shape with zero rows for shots not in Shot_ids.  One GPU, not together with
        pseudo_hessian.  Windowed / band-passed data (if_win, filter) are served: misfit and gradients are those of the conditioned
        misfit 1/2 |Z (C obs - C syn)|^2, under if_envelope_misfit of the envelope misfit 1/2 |Z (e(C obs) - e(C syn))|^2, under
        if_w2_misfit of the trace-wise W2 misfit 1/2 sum_r w_r W_r, under robust_misfit of the Huber / Cauchy misfit sum phi (include/sepfwi.h, sepfwi_cufd);
        if_cross_misfit and if_src_update are refused (SepFwiError).
        Extension `pseudo_hessian=k` > 0 (include/sepfwi.h, sepfwi_pseudo_hessian_arm): the diagonal pseudo-Hessian of the call's
        shots, accumulated on every k-th forward step -> the five plus [hLambda, hMu, hDen] ((nz, nx) each, summed over devices
        and ranks like the gradients; under torch.distributed through ONE more all-reduce, of the fused [hL | hM | hD] buffer).
        With the default 0 the return value and every launch are those of the reference surface."""
        k = int(pseudo_hessian)
        if exact_adjoint:
            if k:
                raise ValueError("exact_adjoint and pseudo_hessian cannot be combined in one call")
            m, gL, gM, gD, *gS = self._adjoint_exact(Lambda, Mu, Den, Stf, ngpu, Shot_ids, para_fname, with_source=bool(source_gradient))
            return [m, gL, gM, gD, gS[0] if gS else torch.zeros_like(_f32c(Stf, "Stf").cpu())]
        if source_gradient:
            raise ValueError("source_gradient needs exact_adjoint=True (the reference's pass returns its own gStf)")
        kw = {"pseudo_hessian": k} if k else {}     # (not armed: _cufd is called exactly as the reference surface calls it)
        parts = self._split_cufd(1, Lambda, Mu, Den, Stf, ngpu, Shot_ids, para_fname, **kw)
        if _dist.active():
            m, gL, gM, gD, gS_loc, *H = parts[0]
            m, gL, gM, gD = _dist.allreduce_gradients(m, gL, gM, gD)
            gS = torch.zeros_like(_f32c(Stf, "Stf").cpu())
            if _dist.rank() == 0:   # the reference returns GPU 0's buffer only (Torch_Fwi.cpp:102-103)
                gS[: gS_loc.shape[0]] = gS_loc
            if k > 0:
                return [m, gL, gM, gD, gS] + list(_dist.allreduce_sum(H[0]))
            return [m, gL, gM, gD, gS]
        if k > 0:   # the parts' pseudo-Hessians summed like the gradients
            H = parts[0][5]
            for p in parts[1:]:
                H += p[5]
            parts = [p[:5] for p in parts]
        m, gL, gM, gD, gS0 = parts[0]
        m = m.clone()                    # not a view of the fused [gL | gM | gD | misfit] buffer: a kept loss must not pin 3 nz nx floats
        for p in parts[1:]:              # sum of Torch_Fwi.cpp:96-101 (every part already sits on Lambda's device)
            m = m + p[0]
            gL += p[1]
            gM += p[2]
            gD += p[3]
        gS = torch.zeros_like(_f32c(Stf, "Stf").cpu())   # zeros_like(th_stf), rows by local shot position
        gS[: gS0.shape[0]] = gS0
        if k > 0:
            return [m, gL, gM, gD, gS] + list(H)
        return [m, gL, gM, gD, gS]

    def forward(self, Lambda, Mu, Den, Stf, gpu_id, Shot_ids, para_fname, *, pseudo_hessian=0):
        """-> [misfit(1,)]   (fwi_forward, Src/Torch_Fwi.cpp:12-36; calc_id 0 on device gpu_id).
        Extension `pseudo_hessian=k` > 0: -> [misfit, hLambda, hMu, hDen] (see backward; this call's device and shots only)."""
        m, *rest = self._cufd(0, self._session_dev(gpu_id), Lambda, Mu, Den, Stf, _shot_ids(Shot_ids), para_fname,
                              **({"pseudo_hessian": int(pseudo_hessian)} if pseudo_hessian else {}))
        if int(pseudo_hessian) > 0:
            return [m] + list(rest[4])
        return [m]

    def obscalc(self, Lambda, Mu, Den, Stf, ngpu, Shot_ids, para_fname, to_store=False):
        """Writes Shot_{pr,vx,vz,ett}{id}.bin; returns None   (fwi_obscalc, Src/Torch_Fwi.cpp:106-136).
        Extension `to_store=True` (SEPFWI_CALC_OBSERVE_TO_STORE): no files -- the axial-strain gather of every shot goes straight
        into the HBM store of observed data of the session that will later evaluate that shot (same device, same shot split as
        `backward` with the same ngpu / ranks), bit for bit what the file route leaves there."""
        self._split_cufd(3 if to_store else 2, Lambda, Mu, Den, Stf, ngpu, Shot_ids, para_fname)
        if _dist.active():
            _dist.barrier()
        return None

    # -- Born modelling and the Gauss-Newton product (sepfwi_born) -------------------------------
    def _born(self, Lambda, Mu, Den, dLambda, dMu, dDen, Stf, ngpu, Shot_ids, para_fname, components, with_hv, dStf=None):
        if int(ngpu) != 1:
            raise ValueError("born / gauss_newton run on ONE GPU (ngpu = 1): the multi-GPU shot split is not implemented for them")
        if _dist.active():
            raise ValueError("born / gauss_newton do not run under torch.distributed: the multi-rank path is not implemented for them")
        comp_id = {"vx": 0, "vz": 1, "ett": 2}
        components = tuple(components)
        for c in components:
            if c not in comp_id:
                raise ValueError("components must be among 'ett', 'vx', 'vz', got %r" % (c,))
        L = _native.lib()
        v = (dLambda, dMu, dDen)
        if dStf is not None and all(t is None for t in v):
            v = ()
        elif dStf is not None and any(t is None for t in v):
            raise ValueError("with dStf, dLambda, dMu, dDen must all be given or all be None")
        Lambda, Mu, Den, Stf, v, ids, nSteps = _checked(Lambda, Mu, Den, Stf, Shot_ids, para_fname, "the model and its perturbation are", v=v)
        dLambda, dMu, dDen = v if v else (None, None, None)
        nrec = _nrec_per_shot(para_fname, ids)
        gpu_id = self._device_for(Lambda, 0)
        gdev = _gdev(Lambda, gpu_id)
        total = int(sum(nrec)) * nSteps
        bufs = [None, None, None]
        for c in components:
            bufs[comp_id[c]] = torch.zeros(max(total, 1), dtype=torch.float32, device=gdev)
        hv = torch.zeros((3,) + tuple(Lambda.shape), dtype=torch.float32, device=gdev) if with_hv else None
        ds = None if dStf is None else _local_rows(dStf, Stf, ids, gdev)
        stream = _stream_or_sync(Lambda, Stf, gpu_id, sync_current=ds is not None)   # (ds: read with a blocking copy inside the library)
        args = (_native.ptr(bufs[2]), _native.ptr(bufs[0]), _native.ptr(bufs[1]), _native.ptr(hv[0]) if with_hv else None, _native.ptr(hv[1]) if with_hv else None,
                _native.ptr(hv[2]) if with_hv else None, _native.ptr(Lambda), _native.ptr(Mu), _native.ptr(Den), _native.ptr(dLambda), _native.ptr(dMu), _native.ptr(dDen), _native.ptr(Stf), gpu_id,
                int(ids.size), _native.ids_arg(ids), _native.path_arg(para_fname), stream)
        rc = L.sepfwi_born(*args) if ds is None else L.sepfwi_born_src(*args, _native.ptr(ds))
        _native.check(rc)
        out, off = [], 0
        for n in nrec:
            out.append({c: bufs[comp_id[c]][off:off + n * nSteps].view(n, nSteps).to(Lambda.device) for c in components})
            off += n * nSteps
        return out, (None if hv is None else hv.to(Lambda.device))

    def born(self, Lambda, Mu, Den, dLambda, dMu, dDen, Stf, ngpu, Shot_ids, para_fname, components=("ett",), dStf=None):
        """Born modelling J v (include/sepfwi.h, sepfwi_born): the first-order change of every gather for the model perturbation
        v = (dLambda, dMu, dDen), propagated next to the background field -- no finite difference, no step size.
        -> a list with one dict per shot of Shot_ids, component name ("ett", "vx", "vz") -> (nrec, nSteps) float32 on the model's device.
        One GPU only (ngpu = 1, no torch.distributed): ValueError otherwise.
        dStf (sepfwi_born_src): a perturbation of the source time function in Stf's shape (rows of shots not in Shot_ids are not read);
        the gathers are then J [v; ds] = J_m v + J_s ds, and dLambda, dMu, dDen may be None together (v = 0)."""
        return self._born(Lambda, Mu, Den, dLambda, dMu, dDen, Stf, ngpu, Shot_ids, para_fname, components, False, dStf=dStf)[0]

    def gauss_newton(self, Lambda, Mu, Den, dLambda, dMu, dDen, Stf, ngpu, Shot_ids, para_fname, exact=False, dStf=None):
        """The Gauss-Newton Hessian-vector product J^T W J v, summed over Shot_ids -> (hvLambda, hvMu, hvDen), each (nz_pad, nx_pad):
        the gradient `backward` would return at the model if the observed data were syn - J v (W: the misfit weights of the parameter
        file).  Under a parameter file whose live conditioning keys are among if_win and filter the same holds for the conditioned
        misfit: the product is J^T C^T Z C J v (C: `condition`; Z: time sample 0 zeroed).  Under if_envelope_misfit it is the
        Gauss-Newton product of the envelope misfit, J^T C^T D^T Z D C J v with D the derivative of the squared envelope at C of the
        background gather (`data_gn` is its data-space part).  Refused (SepFwiError, SEPFWI_EINVAL) under if_cross_misfit,
        if_src_update or if_w2_misfit (the transport misfit has no least-squares Gauss-Newton form here).  Under robust_misfit it is the IRLS
        form J^T C^T Z W Z C J v, W = psi / r at the background (symmetric, non-negative; not the true Hessian): the call reads the shots'
        observed gathers from the session's store (`data_gn(..., obs=)` is its data-space part).  One GPU only, as born.
        exact=True (include/sepfwi.h, sepfwi_adjoint_exact): J^T is the exact transpose of J instead of the reference's backward pass,
        and the product is P J^T W J P v with P the restriction to Omega (the physical interior without its first row and column; v is
        read there only, hv is 0 elsewhere) -- symmetric, v^T hv = |W^1/2 J P v|^2 to float32 rounding (windowed / band-passed data:
        P J^T C^T Z C J P v, v^T hv = |Z C J P v|^2).  The default leaves every bit as it was.
        dStf (exact=True only; sepfwi_adjoint_exact_src): the source block, in Stf's shape.  u = [P v; ds] -> [P; I] J^T W J u, returned
        as (hvLambda, hvMu, hvDen, hvStf) with hvStf in Stf's shape on the host (zero rows for shots not in Shot_ids); dLambda, dMu,
        dDen may be None together.  With exact=False: ValueError -- the reference's backward pass is not J's transpose."""
        if dStf is not None and not exact:
            raise ValueError("dStf needs exact=True: the reference's backward pass is not the transpose of J")
        if exact:
            v = None if (dStf is not None and dLambda is None and dMu is None and dDen is None) else (dLambda, dMu, dDen)
            return self._adjoint_exact(Lambda, Mu, Den, Stf, ngpu, Shot_ids, para_fname, v=v, dStf=dStf)[1:]
        hv = self._born(Lambda, Mu, Den, dLambda, dMu, dDen, Stf, ngpu, Shot_ids, para_fname, (), True)[1]
        return hv[0], hv[1], hv[2]

    # -- the exact discrete adjoint (sepfwi_adjoint_exact) ----------------------------------------
    def _adjoint_exact(self, Lambda, Mu, Den, Stf, ngpu, Shot_ids, para_fname, v=None, w=None, dStf=None, with_source=False):
        """-> (misfit(1,), gLambda, gMu, gDen) on the model's device.  v: (dLambda, dMu, dDen) for the product; w: one dict per shot,
        component name -> (nrec, nSteps), for J^T w; neither: the exact gradient of the session's misfit.  The shot split is _born's.
        dStf (Stf's shape; the product's source block, v may then be None) or with_source: a fifth entry, the source block of the
        result in Stf's shape on the host.  Without either the call is sepfwi_adjoint_exact's, as before."""
        if int(ngpu) != 1:
            raise ValueError("the exact adjoint runs on ONE GPU (ngpu = 1): the multi-GPU shot split is not implemented for it")
        if _dist.active():
            raise ValueError("the exact adjoint does not run under torch.distributed: the multi-rank path is not implemented for it")
        L = _native.lib()
        if dStf is not None and v is not None and any(t is None for t in v):
            raise ValueError("with dStf, dLambda, dMu, dDen must all be given or all be None")
        Lambda, Mu, Den, Stf, v, ids, nSteps = _checked(Lambda, Mu, Den, Stf, Shot_ids, para_fname, "the model is", v=v or ())
        gpu_id = self._device_for(Lambda, 0)
        gdev = _gdev(Lambda, gpu_id)
        src = dStf is not None or with_source
        ds = None if dStf is None else _local_rows(dStf, Stf, ids, gdev)
        g_loc = torch.zeros((int(ids.size), nSteps), dtype=torch.float32, device=gdev) if src else None
        wbuf = {"ett": None, "vx": None, "vz": None}
        if w is not None:
            w = list(w)
            if len(w) != ids.size:
                raise ValueError("w must hold one dict of gathers per shot of Shot_ids")
            comps = sorted({c for d in w for c in d})
            if not comps or any(c not in wbuf for c in comps):
                raise ValueError("w: components must be among 'ett', 'vx', 'vz', and at least one must be given")
            nrec_of = _nrec_per_shot(para_fname, ids)
            for c in comps:
                rows = []
                for i, d, nrec in zip(ids, w, nrec_of):
                    t = d.get(c)
                    t = torch.zeros((nrec, nSteps), dtype=torch.float32) if t is None else _f32c(torch.as_tensor(t), "w[%r]" % c)
                    if tuple(t.shape) != (nrec, nSteps):
                        raise ValueError("w[%r] of shot %d must be (nrec, nSteps) = (%d, %d), got %s" % (c, int(i), nrec, nSteps, tuple(t.shape)))
                    rows.append(t.to(gdev).reshape(-1))
                wbuf[c] = torch.cat(rows) if rows else torch.zeros(1, dtype=torch.float32, device=gdev)
        g = torch.zeros((3,) + tuple(Lambda.shape), dtype=torch.float32, device=gdev)
        misfit = torch.zeros(1, dtype=torch.float32)
        stream = _stream_or_sync(Lambda, Stf, gpu_id, sync_current=True)   # (w was assembled on this stream; the library may run on its own)
        vp = [_native.ptr(t) for t in v] if v else [None, None, None]
        args = (_native.ptr(misfit), _native.ptr(g[0]), _native.ptr(g[1]), _native.ptr(g[2]), _native.ptr(wbuf["ett"]), _native.ptr(wbuf["vx"]), _native.ptr(wbuf["vz"]), *vp,
                _native.ptr(Lambda), _native.ptr(Mu), _native.ptr(Den), _native.ptr(Stf), gpu_id, int(ids.size), _native.ids_arg(ids), _native.path_arg(para_fname), stream)
        rc = L.sepfwi_adjoint_exact_src(*args, _native.ptr(ds), _native.ptr(g_loc)) if src else L.sepfwi_adjoint_exact(*args)
        _native.check(rc)
        g = g.to(Lambda.device)
        if src:
            return misfit.to(Lambda.device), g[0], g[1], g[2], _global_rows(g_loc, Stf, ids)
        return misfit.to(Lambda.device), g[0], g[1], g[2]

    def born_adjoint(self, Lambda, Mu, Den, w, Stf, ngpu, Shot_ids, para_fname, with_source=False):
        """J^T w with the exact discrete adjoint (include/sepfwi.h, sepfwi_adjoint_exact): w is a list with one dict per shot of
        Shot_ids, component name ("ett", "vx", "vz") -> (nrec, nSteps) float32 -- what `born` returns.  No weights, no sign; column 0
        is ignored; a component needs a weight in the parameter file (ett by default).  -> (gLambda, gMu, gDen), each (nz_pad, nx_pad),
        non-zero on Omega only.  One GPU only, as born.  w is in RAW data space under every parameter file this call accepts: if_win and
        filter change nothing here (compose C and C^T with `condition`); if_cross_misfit and if_src_update are refused.
        with_source=True (sepfwi_adjoint_exact_src): -> (gLambda, gMu, gDen, gStf), gStf = J_s^T w in Stf's shape on the host."""
        return self._adjoint_exact(Lambda, Mu, Den, Stf, ngpu, Shot_ids, para_fname, w=w, with_source=bool(with_source))[1:]

    # -- the conditioning operator of a parameter file (sepfwi_condition) -----------------------------
    def condition(self, d, Shot_ids, para_fname, transpose=False, gpu_id=0):
        """C d (or C^T d with transpose=True) of the parameter file: what the session applies to a synthetic axial-strain gather before
        the residual -- per-channel windows with weights (if_win) or the end taper, then the band-pass (filter), then the apparent-slowness
        (f-k) fan filter across each shot's channels (fk_slowness / fk_mode: include/sepfwi.h, sepfwi_cufd); C^T: the fan filter, the
        band-pass, then the window; the identity when no conditioning key is live.  d: the per-shot dict list that `born` returns (every component of
        every dict is conditioned; a new list comes back), or ONE float32 tensor holding the gathers [nrec_i][nSteps] shot after shot in
        the order of Shot_ids (any shape with that many elements; a new tensor of the same shape and device comes back).  The input
        is never changed.  With it a caller composes J^T C^T Z C J from `born` and `born_adjoint`, which stay in raw data space."""
        if not torch.is_tensor(d):
            d, ids = list(d), _shot_ids(Shot_ids)
            if len(d) != ids.size:
                raise ValueError("d must hold one dict of gathers per shot of Shot_ids")
            comps = sorted({c for g in d for c in g})
            out = [dict() for _ in d]
            for c in comps:   # one call per component: the gathers of the shots that have it, shot after shot
                have = [i for i, g in enumerate(d) if c in g]
                flat = self.condition(torch.cat([_f32c(d[i][c], "d[%r]" % c).reshape(-1) for i in have]), ids[have], para_fname, transpose, gpu_id)
                off = 0
                for i in have:
                    n = d[i][c].numel()
                    out[i][c] = flat[off:off + n].view(d[i][c].shape)
                    off += n
            return out
        (out,), ids, dev, stream = self._data_args((d.clone(),), ("d",), Shot_ids, para_fname, gpu_id)   # (the copy is queued before the stream rule)
        _native.check(_native.lib().sepfwi_condition(_native.ptr(out), int(bool(transpose)), dev, int(ids.size), _native.ids_arg(ids),
                                                     _native.path_arg(para_fname), stream))
        return out

    # -- the misfit of a parameter file in data space (sepfwi_data_misfit, sepfwi_data_gn) ----------------
    def _data_args(self, tensors, names, Shot_ids, para_fname, gpu_id):
        """float32 contiguous gathers of one size on one device, checked against the survey -> (tensors, ids, dev, stream)"""
        ids, dev = _shot_ids(Shot_ids), self._session_dev(gpu_id)
        ts = [_f32c(t, n) for t, n in zip(tensors, names)]
        if any(t.numel() != ts[0].numel() or t.device != ts[0].device for t in ts):
            raise ValueError("%s must hold the same number of elements on one device" % " and ".join(names))
        dims = _para_dims(para_fname)
        if dims is not None:
            want = int(sum(_nrec_per_shot(para_fname, ids))) * dims[2]
            if ts[0].numel() != want:
                raise ValueError("%s must hold (nrec_i, nSteps = %d) float32 per shot of Shot_ids, %d elements in all, got %d"
                                 % (names[0], dims[2], want, ts[0].numel()))
        return ts, ids, dev, _stream_for(ts[0], dev)

    def data_misfit(self, obs, syn, Shot_ids, para_fname, gpu_id=0):
        """The parameter file's misfit of RAW axial-strain gathers, with no wave propagation (include/sepfwi.h, sepfwi_data_misfit):
        obs, syn are float32 tensors holding the gathers [nrec_i][nSteps] shot after shot in the order of Shot_ids (any shape with that
        many elements, CPU or HIP).  -> (misfit, adj): the misfit as `forward` reports it (a Python float) and the raw-space adjoint source
        a = -d misfit / d syn in syn's shape and device -- C^T Z (C obs - C syn) under an L2 file, the cross-correlation's under
        if_cross_misfit, C^T D^T Z (e(C obs) - e(C syn)) under if_envelope_misfit, -1/2 C^T w dW / d(C syn) under if_w2_misfit (the
        trace-wise quadratic Wasserstein distance W of include/sepfwi.h, sepfwi_cufd; double arithmetic, rounded once), C^T Z psi under robust_misfit (the Huber / Cauchy penalty with the per-trace quantile scale, csrc/robust_misfit.hpp).  Under if_src_update the matching filter is computed
        from the call's own (C obs, C syn), shot by shot; the misfit is that of the updated synthetics and a holds the filter fixed.
        C includes the fan filter across each shot's channels under fk_slowness / fk_mode (C = FK . band-pass . window), under every kind.
        With `born_adjoint` a caller composes a gradient pass: g = -J^T a."""
        (obs, syn), ids, dev, stream = self._data_args((obs, syn), ("obs", "syn"), Shot_ids, para_fname, gpu_id)
        adj = torch.empty_like(syn)
        mis = C.c_float(0.0)
        _native.check(_native.lib().sepfwi_data_misfit(C.cast(C.byref(mis), C.c_void_p), _native.ptr(adj), _native.ptr(obs), _native.ptr(syn), dev, int(ids.size),
                                                       _native.ids_arg(ids), _native.path_arg(para_fname), stream))
        return float(mis.value), adj

    def data_gn(self, syn, d, Shot_ids, para_fname, gpu_id=0, obs=None):
        """The Gauss-Newton operator of the parameter file's misfit in data space, at syn, applied to d (sepfwi_data_gn): C^T Z C d under
        an L2 file, C^T D^T Z D C d under if_envelope_misfit (D the derivative of the squared envelope at C syn).  Layout as data_misfit;
        -> a new tensor like d.  C includes the fan filter under fk_slowness / fk_mode, as in `condition`.  Symmetric and non-negative;
        refused under if_cross_misfit, if_src_update and if_w2_misfit.  `born`, this and
        `born_adjoint` compose the product J^T (.) J v.
        obs (the observed gathers, laid out like syn): the call goes to sepfwi_data_gn_obs, the operator at (obs, syn).  Under robust_misfit
        it is C^T Z W Z C d with the IRLS weight W of (C obs, C syn) (csrc/robust_misfit.hpp) and obs is required -- without it the library
        refuses (SepFwiError) and names that entry; under every other file the result is the one without obs, bit for bit."""
        if obs is not None:
            (obs, syn, d), ids, dev, stream = self._data_args((obs, syn, d), ("obs", "syn", "d"), Shot_ids, para_fname, gpu_id)
            out = torch.empty_like(d)
            _native.check(_native.lib().sepfwi_data_gn_obs(_native.ptr(out), _native.ptr(obs), _native.ptr(syn), _native.ptr(d), dev, int(ids.size),
                                                           _native.ids_arg(ids), _native.path_arg(para_fname), stream))
            return out
        (syn, d), ids, dev, stream = self._data_args((syn, d), ("syn", "d"), Shot_ids, para_fname, gpu_id)
        out = torch.empty_like(d)
        _native.check(_native.lib().sepfwi_data_gn(_native.ptr(out), _native.ptr(syn), _native.ptr(d), dev, int(ids.size), _native.ids_arg(ids),
                                                   _native.path_arg(para_fname), stream))
        return out

    # -- extras --------------------------------------------------------------------------------
    def set_observed(self, para_fname, shot_id, ett, gpu_id=0):
        """Observed axial-strain gather of one shot from a tensor ((nrec, nSteps) float32, CPU or HIP) instead of
        Shot_ett{id}.bin: cached in HBM by the session of (para_fname, gpu_id) until release() / invalidation."""
        ett = _f32c(ett, "ett")
        if ett.dim() != 2:
            raise ValueError("ett must be (nrec, nSteps)")
        if ett.is_cuda:     # the library copies on its own stream, ordered only behind the legacy default stream
            torch.cuda.current_stream(ett.device).synchronize()
        _native.check(_native.lib().sepfwi_set_observed(_native.path_arg(para_fname), self._session_dev(gpu_id), int(shot_id), _native.ptr(ett),
                                                        int(ett.shape[0]), int(ett.shape[1])))

    def set_observed_component(self, para_fname, shot_id, comp, data, gpu_id=0):
        """Observed gather of one shot and component from a tensor ((nrec, nSteps) float32, CPU or HIP) instead of
        Shot_{vx,vz,ett}{id}.bin, for a joint misfit (parameter keys misfit_w_*): comp "vx" / "vz" / "ett" or 1 / 2 / 3."""
        comp = {"vx": 1, "vz": 2, "ett": 3}.get(comp, comp)
        data = _f32c(data, "data")
        if data.dim() != 2:
            raise ValueError("data must be (nrec, nSteps)")
        if data.is_cuda:
            torch.cuda.current_stream(data.device).synchronize()
        _native.check(_native.lib().sepfwi_set_observed_component(_native.path_arg(para_fname), self._session_dev(gpu_id), int(shot_id), int(comp), _native.ptr(data),
                                                                  int(data.shape[0]), int(data.shape[1])))

    def misfit_parts(self, para_fname, gpu_id=0):
        """{"vx", "vz", "ett"}: the unweighted 0.5 sum r_c^2 of the session's last misfit or gradient call (sepfwi_get_misfit_parts;
        0 for a component with weight 0; this process's shots only)."""
        parts = (C.c_double * 3)()
        _native.check(_native.lib().sepfwi_get_misfit_parts(_native.path_arg(para_fname), self._session_dev(gpu_id), parts))
        return {"vx": parts[0], "vz": parts[1], "ett": parts[2]}

    def debug_field(self, para_fname, which, lane=0, gpu_id=0):
        """Test hook (sepfwi_debug_field): wavefield 0..4 (vz, vx, szz, sxx, sxz) / adjoint 5..9 of a forward lane as the
        last call left it, (nz - nPad, nx) float32."""
        j = _utils.read_para(para_fname)
        out = torch.empty((int(j["nz"]) - int(j["nPad"]), int(j["nx"])), dtype=torch.float32)
        _native.check(_native.lib().sepfwi_debug_field(_native.path_arg(para_fname), self._session_dev(gpu_id), int(lane), int(which), _native.ptr(out)))
        return out

    def stats(self, para_fname, gpu_id=0):
        st = _native.Stats()
        _native.check(_native.lib().sepfwi_get_stats(_native.path_arg(para_fname), int(gpu_id), C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def loop_status(self, para_fname, gpu_id=0):
        """"" while the session's backward passes run in the persistent loop, else why they do not (sepfwi_loop_status)."""
        buf = C.create_string_buffer(512)
        _native.check(_native.lib().sepfwi_loop_status(_native.path_arg(para_fname), int(gpu_id), buf, 512))
        return buf.value.decode(errors="replace")

    def release(self):
        _native.lib().sepfwi_release_all()


fwi_ops = _FwiOps()


class FWIFunction(torch.autograd.Function):
    """forward() runs forward+adjoint and caches the gradients; backward() hands them out and ignores
    grad_misfit -- exactly the reference behaviour (FWI_ops.py:46-63)."""

    @staticmethod
    def forward(ctx, Lambda, Mu, Den, Stf, ngpu, Shot_ids, para_fname):
        from . import ops as _self   # late lookup so tests may swap `fwi_ops`
        outputs = _self.fwi_ops.backward(Lambda, Mu, Den, Stf, ngpu, Shot_ids, para_fname)
        ctx.outputs = outputs[1:]
        return outputs[0]

    @staticmethod
    def backward(ctx, grad_misfit):
        grad_Lambda, grad_Mu, grad_Den, grad_stf = ctx.outputs
        return grad_Lambda, grad_Mu, grad_Den, grad_stf, None, None, None
