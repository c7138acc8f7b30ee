"""What the tests of the data-space entry points share (fwi_ops.data_misfit / data_gn with no time loop: tests/test_gpu_envelope_data.py,
tests/test_gpu_cross_data.py, tests/test_gpu_source_update_data.py): a parameter / survey file pair with a given channel count per shot,
seeded band-limited traces for it, and the flat layout of the gathers."""
import numpy as np
import torch

import cond_gn_ref as G
import envelope_ref as E
import problems as P

DT = 1.0e-3
NSTEPS = (2, 3, 63, 64, 65, 255, 256, 257, 600)      # the per-trace reduction's wavefront (64) and block (256) edges, the shortest transforms


def problem(tmp, nt, nrec, keys, name, misfit_key=E.KEY, nx=48):
    """a parameter / survey file pair: len(nrec) shots with nrec[i] channels on a 40 x nx grid with 10-cell layers (nothing propagates: only
    the channel counts matter, and nx has to hold them: 6 + max(nrec) <= nx), windows and weights in the survey (channel 1 has weight 0, the
    last channel of a shot with three or more an empty window: "Window error 1", its trace passes untouched), `keys` and the misfit's key in
    the parameter file"""
    assert 6 + max(nrec) <= nx
    pb = P.make_problem(str(tmp), nz=40, nx=nx, nPml=10, nSteps=nt, nshots=len(nrec), dt=DT, rec_x=list(range(6, 6 + max(nrec))))
    rng = np.random.default_rng(17)
    sv, T = dict(pb["survey"]), nt * DT
    for i, n in enumerate(nrec):
        sh = dict(sv["shot%d" % i])
        sh["z_rec"], sh["x_rec"], sh["nrec"] = sh["z_rec"][:n], sh["x_rec"][:n], n
        sh["win_start"] = [float(v) for v in rng.uniform(0.05 * T, 0.3 * T, n)]
        sh["win_end"] = [float(v) for v in rng.uniform(0.6 * T, 0.95 * T, n)]
        sh["weights"] = [float(v) for v in rng.uniform(0.5, 2.0, n)]
        if n > 1:
            sh["weights"][1] = 0.0
        if n >= 3:
            sh["win_end"][n - 1] = sh["win_start"][n - 1]
        sh["src_weight"] = 1.3 + 0.2 * i
        sv["shot%d" % i] = sh
    para = dict({k: v for k, v in pb["para"].items() if k not in E.STRIP}, **keys)
    if misfit_key:
        para[misfit_key] = True
    pb = dict(pb)
    pb["para_fname"], pb["para"] = G.write_files(pb, name, para, sv)
    pb["survey"] = sv
    return pb


def traces(pb, seed, amp=1.0):
    """per shot a (nrec, nSteps) float32 gather of band-limited traces with peaks 0.5 ... 1.5 times amp"""
    nt = pb["nSteps"]
    rng = np.random.default_rng(seed)
    out = [E.band_limited(rng, int(pb["survey"]["shot%d" % s]["nrec"]), nt) for s in G.shots_of(pb)]
    return out if amp == 1.0 else [(np.float32(amp) * g).astype(np.float32) for g in out]


def flat(gathers):
    return torch.from_numpy(np.concatenate([np.asarray(g, np.float32).reshape(-1) for g in gathers]))


def unflat(t, like):
    a, out, off = t.cpu().numpy(), [], 0
    for g in like:
        out.append(a[off:off + g.size].reshape(g.shape))
        off += g.size
    return out


def rel(got, ref):
    return G.norm([np.asarray(a, np.float64) - np.asarray(b, np.float64) for a, b in zip(got, ref)]) / G.norm(ref)
