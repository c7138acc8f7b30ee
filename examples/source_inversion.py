#!/usr/bin/env python
"""Inversion of the source time function alone, with the model fixed at the true one: the wavelet starts wrong in amplitude and shifted
in time, and a few matrix-free conjugate-gradient iterations on the source block of the Gauss-Newton operator recover it,
    H_ss p = -g,      g = d misfit / d Stf  (fwi_ops.backward(exact_adjoint=True, source_gradient=True)),
                      H_ss p = J_s^T W J_s p  (fwi_ops.gauss_newton(None, None, None, ..., exact=True, dStf=p)),
through sepfwi.obj_wrapper.gauss_newton_cg, which works on tuples of tensors of any shape.  The wavefield is exactly linear in the source,
so the misfit is exactly quadratic in Stf and the Gauss-Newton operator is its Hessian: the misfit along the CG iterates never increases.
An extension without a counterpart in the reference, whose only route to a wavelet is its inexact backward pass.

    python examples/source_inversion.py --device cuda
    python examples/source_inversion.py --device cuda --small

Prints the misfit at every CG iterate (one extra misfit call each) and the misfit before and after."""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sep-2023_amd")]
from sepfwi import utils as ft            # noqa: E402
from sepfwi import fwi_ops                # noqa: E402
from sepfwi.obj_wrapper import gauss_newton_cg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=6, help="conjugate-gradient iterations")
    ap.add_argument("--small", action="store_true", help="a 44 x 60 grid, 240 steps, 2 shots instead of 101 x 201, 1001 steps, 4 shots")
    ap.add_argument("--device", default="cpu", choices=["cpu", "cuda"], help="where the model tensors live")
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    dev = torch.device(a.device)

    if a.small:
        nz, nx, dh, dt, nt, f0, nPml, nshots, shift = 44, 60, 10.0, 1.0e-3, 240, 25.0, 10, 2, 6
    else:
        nz, nx, dh, dt, nt, f0, nPml, nshots, shift = 101, 201, 20.0, 2.0e-3, 1001, 10.0, 32, 4, 12
    vp = np.ones((nz, nx), np.float32) * 3500.0
    vp[nz // 2 - 6:nz // 2 + 6, nx // 3 - 6:nx // 3 + 6] += 250.0      # the model is known: the true one, with its anomaly
    vs = vp / 1.732
    rho = np.ones((nz, nx), np.float32) * 2400.0
    nPad = ft.nPad_for(nz, nPml)
    nz_pad, nx_pad = nz + 2 * nPml + nPad, nx + 2 * nPml
    src_x = np.linspace(8, nx - 9, nshots).round().astype(int)
    rec_x = np.arange(4, nx - 4).astype(int)
    work = a.workdir or os.path.join(tempfile.gettempdir(), "sepfwi_example_source_inversion")
    os.makedirs(work, exist_ok=True)
    para_fname, survey_fname = os.path.join(work, "para_file.json"), os.path.join(work, "survey_file.json")
    ft.paraGen(nz_pad, nx_pad, dh, dh, nt, dt, f0, nPml, nPad, para_fname, survey_fname, os.path.join(work, "Data"))
    ft.surveyGen(2 * np.ones_like(src_x), src_x, (nz - 6) * np.ones_like(rec_x), rec_x, survey_fname)
    ids = torch.arange(nshots, dtype=torch.int32)
    t = [torch.tensor(ft.padding_numpy_array(m, nPml, nPad), dtype=torch.float32, device=dev) for m in (vp, vs, rho)]
    m = [((t[0] ** 2 - 2.0 * t[1] ** 2) * t[2] / 1e6).contiguous(), (t[1] ** 2 * t[2] / 1e6).contiguous(), t[2].contiguous()]

    ricker = torch.tensor(ft.sourceGene(f0, nt, dt), dtype=torch.float32)
    Stf_true = ricker.repeat(nshots, 1)
    Stf = (0.6 * torch.roll(ricker, shift)).repeat(nshots, 1).contiguous()      # wrong in amplitude, late by `shift` samples
    Stf[:, :shift] = 0.0
    fwi_ops.obscalc(*m, Stf_true, 1, ids, para_fname, to_store=True)            # observed data straight into the session's store

    misfit = lambda s: float(fwi_ops.forward(*m, s.contiguous(), 0, ids, para_fname)[0])
    out = fwi_ops.backward(*m, Stf, 1, ids, para_fname, exact_adjoint=True, source_gradient=True)
    f_start, g = float(out[0]), out[4]
    print("cg 0: misfit %.6e" % f_start, flush=True)

    # CG is deterministic: the j-th product of a run capped at k iterations is the j-th of every longer run.  The products are kept, so
    # the iterate after every iteration (gauss_newton_cg returns the last one only) costs no product twice.
    kept = []

    def solve(k):
        calls = [0]

        def hv(v):
            j, calls[0] = calls[0], calls[0] + 1
            if j == len(kept):
                kept.append(fwi_ops.gauss_newton(*m, None, None, None, Stf, 1, ids, para_fname, exact=True, dStf=v[0])[3])
            return (kept[j],)

        return gauss_newton_cg(hv, (g,), maxiter=k, rtol=0.0)

    f, p = f_start, None
    for k in range(1, a.iters + 1):
        (p,), hist = solve(k)
        if len(hist) - 1 < k:      # the solve ended early (no curvature left along the search direction)
            break
        f = misfit(Stf + p)
        print("cg %d: misfit %.6e   (relative residual %.3e)" % (k, f, hist[-1]), flush=True)
    err = lambda s: float((s - Stf_true).norm() / Stf_true.norm())
    print("done: misfit %.4e -> %.4e (ratio %.3e); wavelet error |stf - true| / |true| %.3f -> %.3f" % (f_start, f, f / f_start, err(Stf), err(Stf + p)))


if __name__ == "__main__":
    main()
