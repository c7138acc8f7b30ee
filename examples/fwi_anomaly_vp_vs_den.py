#!/usr/bin/env python
"""Vp/Vs/density FWI of the three-box anomaly model with DAS data -- the reference's experiment 001
(DAS_Waveform_Inversion/notebooks/001-FWI-Anomaly-Vp-Vs-Den.ipynb cells 3,7 + Main-001-...py:20-168) with only the
import changed: `from sepfwi import ...` instead of the reference's `FWI_ops` / `fwi_utils` / `obj_wrapper`.

    python examples/fwi_anomaly_vp_vs_den.py --niter 10                 # host tensors, like the reference
    python examples/fwi_anomaly_vp_vs_den.py --niter 10 --device cuda   # every tensor of the iteration in HBM
    torchrun --nproc-per-node 8 examples/fwi_anomaly_vp_vs_den.py       # shots sharded over 8 GPUs, one all-reduce
    python examples/fwi_anomaly_vp_vs_den.py --device cuda --precond 1e-3   # L-BFGS-B on variables scaled by the pseudo-Hessian
    python examples/fwi_anomaly_vp_vs_den.py --device cuda --smooth 60      # L-BFGS in y, the model p_ref + s S y, S a 60 m Gaussian

Model files of the reference are replaced by their analytic definition (homogeneous + three 16x16-cell boxes).
The printed iterate-0 misfit is the reference's own 1.51116e4 (tests/golden/known_answers.json)."""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch
from scipy import optimize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sep-2023_amd")]
from sepfwi import dist as fdist          # noqa: E402
from sepfwi import modules as M           # noqa: E402
from sepfwi import utils as ft            # noqa: E402
from sepfwi import fwi_ops                # noqa: E402
from sepfwi.obj_wrapper import PyTorchObjective, minimize_lbfgsb  # noqa: E402


def pseudo_hessian_scale(fwi, Stf, Shot_ids, ngpu, para_fname, eps):
    """One armed evaluation at the start model -> the scale vector of minimize_lbfgsb, ordered like the module's parameters:
    per parameter (H + eps max H)^(-1/2) on the physical grid, normalised to median 1 (H: the diagonal pseudo-Hessian of the call's
    shots mapped to Vp / Vs / Den, a source-side illumination -- an extension without a counterpart in the reference)."""
    with torch.no_grad():
        vp, vs, den = fwi._masked()
        lam, mu, rho = fwi.lame(vp, vs, den)
        out = fwi_ops.backward(lam.contiguous(), mu.contiguous(), rho.contiguous(), Stf, ngpu, Shot_ids, para_fname, pseudo_hessian=1)
        H = ft.pseudo_hessian_vp_vs_den(*[h.to(vp.device) for h in out[5:8]], vp, vs, den)
    z0, x0 = fwi.nPml, fwi.nPml
    by_name = dict(zip(fwi.NAMES, H))
    parts = []
    for name, _ in fwi.named_parameters():
        h = by_name[name][z0:z0 + fwi.nz_orig, x0:x0 + fwi.nx_orig].double().cpu().numpy()
        sc = (h + eps * h.max()) ** -0.5
        parts.append((sc / np.median(sc)).ravel())
    return np.concatenate(parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--niter", type=int, default=5)
    ap.add_argument("--device", default="cpu", choices=["cpu", "cuda"], help="where the model tensors live")
    ap.add_argument("--ngpu", type=int, default=1, help="devices driven by this process (ignored under torchrun)")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--precond", type=float, default=None, metavar="EPS",
                    help="scale the variables by (H + EPS max H)^(-1/2), H the diagonal pseudo-Hessian of the start model (default: off)")
    ap.add_argument("--smooth", type=float, default=None, metavar="METRES",
                    help="invert in the smoothed variables y, the model p_ref + s S y with S a Gaussian of this width (sepfwi.smooth; no bounds) (default: off)")
    a = ap.parse_args()
    if a.smooth is not None and a.precond is not None:
        ap.error("--precond scales the model variables, --smooth replaces them: use one")
    if "RANK" in os.environ:   # one process per GPU
        import torch.distributed as td
        torch.cuda.set_device(int(os.environ["LOCAL_RANK"]))
        td.init_process_group(backend="nccl")
    rank = fdist.rank() if fdist.active() else 0
    dev = torch.device(a.device if not fdist.active() else "cuda")

    # ---- model and survey: Main-001-...py:20-73
    nx, nz, dx, dz, dt, nt, f0, nPml = 201, 101, 20.0, 20.0, 0.002, 1501, 10.0, 32
    vp = np.ones((nz, nx), np.float32) * 4000.0
    vs = vp / 1.732
    rho = np.ones((nz, nx), np.float32) * 2500.0
    vp0, vs0, rho0 = vp.copy(), vs.copy(), rho.copy()
    vp[42:58, 42:58] += 80.0
    vs[42:58, 92:108] -= 80.0 / 1.732
    rho[42:58, 142:158] += 40.0
    nPad = ft.nPad_for(nz, nPml)
    nz_pad, nx_pad = nz + 2 * nPml + nPad, nx + 2 * nPml
    Mask = np.zeros((nz_pad, nx_pad), np.float32)
    Mask[nPml:nPml + nz, nPml:nPml + nx] = 1.0
    Mask[nPml:nPml + 4, :] = 0.0
    ind_src_x = np.arange(10, nx - 10, 10).astype(int)
    ind_src_z = np.ones_like(ind_src_x)
    ind_rec_x = np.arange(10, nx - 10).astype(int)
    ind_rec_z = 95 * np.ones_like(ind_rec_x)

    work = a.workdir or os.path.join(tempfile.gettempdir(), "sepfwi_example_001")
    os.makedirs(work, exist_ok=True)
    para_fname, survey_fname = os.path.join(work, "para_file.json"), os.path.join(work, "survey_file.json")
    if rank == 0:
        ft.paraGen(nz_pad, nx_pad, dz, dx, nt, dt, f0, nPml, nPad, para_fname, survey_fname, os.path.join(work, "Data"))
        ft.surveyGen(ind_src_z, ind_src_x, ind_rec_z, ind_rec_x, survey_fname)
    if fdist.active():
        fdist.barrier()
    Stf = torch.tensor(ft.sourceGene(f0, nt, dt), dtype=torch.float32).repeat(len(ind_src_x), 1).to(dev)
    Shot_ids = torch.arange(len(ind_src_x), dtype=torch.int32)
    opt = dict(nz=nz, nx=nx, nz_orig=nz, nx_orig=nx, nPml=nPml, nPad=nPad, para_fname=para_fname)

    # ---- observed data from the true model: Main-001-...py:96-110
    pad = lambda m: torch.tensor(ft.padding_numpy_array(m, nPml, nPad), dtype=torch.float32, device=dev)
    M.FWI_obscalc(pad(vp), pad(vs), pad(rho), Stf, para_fname)(Shot_ids, ngpu=a.ngpu)

    # ---- inversion: Main-001-...py:112-168
    T = lambda m: torch.tensor(m, dtype=torch.float32, device=dev, requires_grad=True)
    fwi = M.FWI(T(vp0), T(vs0), T(rho0), Stf, opt, Mask=torch.tensor(Mask, device=dev))
    if a.smooth is not None:
        from sepfwi.smooth import Smoother
        obj = PyTorchObjective(fwi, lambda: fwi(Shot_ids, ngpu=a.ngpu), smoother=Smoother(fwi, a.smooth, a.smooth))
    else:
        obj = PyTorchObjective(fwi, lambda: fwi(Shot_ids, ngpu=a.ngpu))
    fun, jac = obj.fun, obj.jac   # bound methods (cache() later shadows .jac with the array, as in the reference)
    hist = [fun(obj.x0)]
    if rank == 0:
        print("iterate 0: misfit %.6e   |proj g|_inf %.6e" % (hist[0], np.abs(jac(obj.x0)).max()))

    def cb(x):
        hist.append(obj.f)
        if rank == 0:
            print("iterate %d: misfit %.6e" % (len(hist) - 1, obj.f), flush=True)

    if a.precond is not None:
        scale = pseudo_hessian_scale(fwi, Stf, Shot_ids, a.ngpu, para_fname, a.precond)
        if rank == 0:
            print("preconditioner: scale min %.3e max %.3e (median 1 per parameter)" % (scale.min(), scale.max()), flush=True)
        res = minimize_lbfgsb(fun, obj.x0, jac, bounds=obj.bounds, callback=cb, gtol=1e-16, maxiter=a.niter, ftol=1e-12, maxcor=5,
                              maxfun=1500, maxls=6, scale=scale)
    else:
        res = optimize.minimize(fun, obj.x0, method="L-BFGS-B", jac=jac, bounds=obj.bounds, tol=None, callback=cb,
                                options={"gtol": 1e-16, "maxiter": a.niter, "ftol": 1e-12, "maxcor": 5, "maxfun": 1500, "maxls": 6})
    if rank == 0:
        n = nz * nx
        if a.smooth is not None:      # res.x is y: the model is the module's, loaded at y
            obj.load(res.x)
            dvp = fwi.Vp.detach().cpu().numpy() - vp0
        else:
            dvp = res.x[:n].reshape(nz, nx) - vp0
        print("done: %d evaluations, misfit %.4e -> %.4e; recovered Vp anomaly peak %.1f m/s (true 80)" %
              (res.nfev, hist[0], hist[-1], dvp[42:58, 42:58].max()))
    if fdist.active():
        import torch.distributed as td
        td.destroy_process_group()


if __name__ == "__main__":
    main()
