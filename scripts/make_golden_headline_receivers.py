#!/usr/bin/env python
"""tests/golden/oracle_headline_receivers_<case>.npz: the headline grid (2000 x 1000 cells + 32-cell layers, padded 2064 x 1088)
with receivers that are NOT a fused horizontal line, one shot, 400 time steps, forward + boundary-saving adjoint through the CPU
oracle (oracle/torchfwi_oracle.c).  At this size the shipped backward pass is the persistent loop in strip order, and these
receivers reach it through the folded adjoint source (k_inject_values + the GINJ branch of k_bwd_persist);
tests/test_gpu_headline.py::test_headline_grid_general_receivers compares the HIP path with these files.

Cases (CASES below):
  stride3      a horizontal line with a channel every third cell
  vertical     a vertical fibre (ezz) in column nx/2 + 3, the source 20 columns beside it
  directional  every other cell of a horizontal line, every channel its own direction cosines
  bandpass     the channels of `stride3` with the residual band-passed (para "filter" = [3, 7, 40, 60] Hz)
  gauge4       the channels of `stride3` with a gauge length of four cells (para "das_gauge_length" = 4 dx): even G, five members,
               neighbouring gauges overlap, four taps per channel, targets on both sides of 64-column segment boundaries.  The oracle
               runs the expanded member survey (tests/gauge_ref.py); observed data are the true model's gauge gathers

Geometry: the source and the horizontal lines sit at one of the seams between the persistent loop's eight XCD bands (padded row
round(b nzc / 8), persist_plan.cpp), the source two rows above it and the line on its first row below, so the wave and the
adjoint source cross the seam, and the directional channels' stencils straddle it.  The vertical fibre crosses every seam.

About 4e9 cell-updates per case (the band-passed one runs one forward more).

    python scripts/make_golden_headline_receivers.py                      # all four golden files
    python scripts/make_golden_headline_receivers.py --case vertical      # one of them
    python scripts/make_golden_headline_receivers.py --nsteps 60 --out calib.npz --case stride3   # a short calibration run

Stored (decimated, < 1 MB each): 64 channels of the observed ("true" model) and synthetic (trial model) axial-strain gathers,
misfit, every 8th cell of the three gradients, two full-resolution 96 x 96 windows of each (under the source; where the channels
cross the seam), the source-function gradient, norms and peaks, the residual energy per channel, and a digest of the inputs
(models, source function, survey and parameter file) so a drift of the problem generator is detected without the oracle."""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sep-2023_amd"), os.path.join(ROOT, "tests")]
import problems as P  # noqa: E402

NZ, NX, NPML, NSTEPS = 1000, 2000, 32, 400
CASES = ("stride3", "vertical", "directional", "bandpass", "gauge4")
GAUGE = 4
FILTER = [3.0, 7.0, 40.0, 60.0]
NBAND = 8                     # XCD bands of the persistent loop on an MI355X
SEAM_BAND = 4                 # the seam between bands 3 and 4 (mid-depth: the make_problem anomalies are there)
DECIM = 8
WIN = 96
NCH = 64


def golden_path(case):
    return os.path.join(ROOT, "tests", "golden", "oracle_headline_receivers_%s.npz" % case)


def seams(nz_pad, nPad, nband=NBAND):
    """Padded rows where the persistent loop's bands start (make_persist_plan with equal band weights: row0[b] = round(b nzc / nband))."""
    nzc = nz_pad - nPad
    return [int(b / nband * nzc + 0.5) for b in range(1, nband)]


def geometry(case, nsteps=NSTEPS):
    """make_problem arguments of a case, and the seam (padded row) it is placed at."""
    from sepfwi import utils as ft
    nPad = ft.nPad_for(NZ, NPML)
    seam = seams(NZ + 2 * NPML + nPad, nPad)[SEAM_BAND - 1]
    src_z, line_z = seam - 2 - NPML, seam - NPML          # unpadded rows: source in band SEAM_BAND-1, line on band SEAM_BAND's first row
    kw = dict(nz=NZ, nx=NX, nPml=NPML, nSteps=nsteps, nshots=1, hetero=True, seed=3)
    if case in ("stride3", "bandpass", "gauge4"):
        kw.update(nrec_stride=3, rec_z=line_z, src_z=src_z, src_x=[NX // 2])
    elif case == "vertical":
        kw.update(das_fiber="vertical", src_z=src_z, src_x=[NX // 2 + 3 - 20])
    elif case == "directional":
        kw.update(das_sensitivity="random", nrec_stride=2, rec_z=line_z, src_z=src_z, src_x=[NX // 2])
    else:
        raise ValueError(case)
    return kw, seam


def make_case(workdir, case, nsteps=NSTEPS):
    """The problem of a case (problems.make_problem + the band-pass filter in the parameter file).  Adds the seam row and the
    padded-grid windows: `win_src` under the source, `win_seam` where the channels cross the seam."""
    kw, seam = geometry(case, nsteps)
    pb = P.make_problem(workdir, **kw)
    # the trial model: lambda 5 % above the smooth initial one, so the residual is of the size of the data from the first arrival on.
    # (With only make_problem's small anomalies as residual, the direct wave two rows from the source dominates the data, and the
    # round-off of the observed data -- modelled by the library under test on the GPU -- sets the source gradient's error.)
    lam, mu, den = pb["lame_init"]
    pb["lame_init"] = ((lam * 1.05).contiguous(), mu, den)
    if case == "bandpass":
        pb["para"]["filter"] = FILTER
        with open(pb["para_fname"], "w") as fp:
            json.dump(pb["para"], fp)
    if case == "gauge4":
        pb["para"]["das_gauge_length"] = GAUGE * pb["para"]["dx"]
        with open(pb["para_fname"], "w") as fp:
            json.dump(pb["para"], fp)
    sh = pb["survey"]["shot0"]
    sz, sx = int(sh["z_src"]) + NPML, int(sh["x_src"]) + NPML
    h = WIN // 2
    pb["seam"] = seam
    pb["win_src"] = (sz - h, sz + h, sx - h, sx + h)
    cx = NX // 2 + 3 + NPML if case == "vertical" else sx + 64      # the fibre's column / along the line beside the source
    pb["win_seam"] = (seam - h, seam + h, cx - h, cx + h)
    return pb


def digest(pb):
    """Models, source function, survey and the parameter file's physics (paths left out)."""
    h = hashlib.sha256()
    for t in list(pb["lame_true"]) + list(pb["lame_init"]) + [pb["Stf"]]:
        h.update(np.ascontiguousarray(t.numpy()).tobytes())
    para = {k: v for k, v in pb["para"].items() if k not in ("survey_fname", "data_dir_name", "scratch_dir_name")}
    h.update(json.dumps(para, sort_keys=True).encode())
    h.update(json.dumps(pb["survey"], sort_keys=True).encode())
    return h.hexdigest()


def channels(nrec):
    return np.unique(np.linspace(0, nrec - 1, NCH).round().astype(int))


def run(case, nsteps, out):
    from oracle import oracle as O
    with tempfile.TemporaryDirectory() as d:
        pb = make_case(d, case, nsteps)
        para, survey = pb["para"], pb["survey"]
        plain = {k: v for k, v in para.items() if k != "filter"}
        stf = pb["Stf"].numpy()
        t0 = time.time()
        lam, mu, den = [t.numpy() for t in pb["lame_true"]]
        if case == "gauge4":
            import gauge_ref as R
            obs_ett = R.forward(O, (lam, mu, den), stf, [0], para, survey, GAUGE)[0][0].astype(np.float32)
        else:
            obs = O.cufd(lam, mu, den, stf, 2, [0], plain, survey)["syn"]
            obs_ett = obs[0, 3]
        print("%s observe: %.1f s" % (case, time.time() - t0), flush=True)
        t0 = time.time()
        lam, mu, den = [t.numpy() for t in pb["lame_init"]]
        if case == "gauge4":
            ref = R.reference(O, (lam, mu, den), stf, [0], para, survey, GAUGE, [obs_ett])
            syn_ett = ref["gauge"][0].astype(np.float32)
        else:
            ref = O.cufd(lam, mu, den, stf, 1, [0], para, survey, obs=obs)
            syn_ett = ref["syn"][0, 3]
        print("%s gradient: %.1f s, misfit %.6e" % (case, time.time() - t0, ref["misfit"]), flush=True)
        ch = channels(pb["nrec"])
        r = obs_ett.astype(np.float64) - syn_ett.astype(np.float64)
        out_ = dict(misfit=np.float64(ref["misfit"]), gStf=ref["gStf"][0], digest=digest(pb), channels=ch, decim=DECIM,
                    seam=np.int64(pb["seam"]), win_src=np.array(pb["win_src"]), win_seam=np.array(pb["win_seam"]),
                    obs_ett=obs_ett[ch], syn_ett=syn_ett[ch],
                    obs_ett_norm=np.float64(np.linalg.norm(obs_ett.astype(np.float64))),
                    res_energy=(r * r).sum(axis=1))                 # per channel, unconditioned (obs - syn)
        for k in ("gLambda", "gMu", "gDen"):
            a = ref[k]
            z0, z1, x0, x1 = pb["win_src"]
            w0, w1, v0, v1 = pb["win_seam"]
            out_[k + "_dec"] = np.ascontiguousarray(a[::DECIM, ::DECIM])
            out_[k + "_win_src"] = np.ascontiguousarray(a[z0:z1, x0:x1])
            out_[k + "_win_seam"] = np.ascontiguousarray(a[w0:w1, v0:v1])
            out_[k + "_norm"] = np.float64(np.linalg.norm(a.astype(np.float64)))
            out_[k + "_max"] = np.float64(np.abs(a).max())
        np.savez_compressed(out, **out_)
        print("wrote", out, os.path.getsize(out), "bytes", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES, action="append")
    ap.add_argument("--nsteps", type=int, default=NSTEPS)
    ap.add_argument("--out", default=None, help="output file (one --case only)")
    args = ap.parse_args()
    cases = args.case or list(CASES)
    if args.out is not None and len(cases) != 1:
        raise SystemExit("--out needs exactly one --case")
    golden_dir = os.path.join(ROOT, "tests", "golden")
    if args.nsteps != NSTEPS and (args.out is None or os.path.abspath(args.out).startswith(golden_dir)):
        raise SystemExit("a shortened run is not a golden file: give --out somewhere else")
    from oracle import oracle as O
    O.build()
    for case in cases:
        run(case, args.nsteps, args.out or golden_path(case))


if __name__ == "__main__":
    main()
