"""The reference for the normalised zero-lag cross-correlation misfit (parameter key if_cross_misfit; csrc/conditioning.hip: k_normfact,
k_cross_misfit, k_cross_adjoint), outside the GPU: numpy, float64 on float32 inputs.

Per shot, for the conditioned gathers o = C obs, s = C syn and the trace weights w_r = weights[r] * src_weight (1 without if_win):
    n_xy     sum_t x y + DIVCONST, DIVCONST the float32 value of 1e-9f (the constant the kernel adds; absolute, so the definition depends
             on the data's amplitude)
    cc_r     n_os / (sqrt(n_oo) sqrt(n_ss)), the normalised correlation of trace r
    misfit   1/2 (-2 sum_r w_r cc_r)
    a        the adjoint source the propagator injects, -d misfit / d syn = C^T [ w_r (o - (n_os / n_ss) s) / (sqrt(n_oo) sqrt(n_ss)) ]
Sample 0 is not zeroed in this branch, as in the kernel.

C and C^T are the oracle's (cond_gn_ref.C_of / Ct_of: window, then band-pass / band-pass, then window; under the key alone the plain end
taper); either oracle build serves, and the distance between the two is the yardstick of the band-passed cases.  oracle.conditioned_residual
restates the same expressions in float32, norms included: on nearly fitting data (obs close to a multiple of syn) the difference
o - (n_os / n_ss) s is a cancellation, and the float32 restatement is then no yardstick -- this one is (tests/test_cross_reference.py
measures by how much)."""
import numpy as np

import cond_gn_ref as G

KEY = "if_cross_misfit"
DIVCONST = float(np.float32(1e-9))


# ---- the definitions, on (nrec, nt) arrays ----------------------------------------------------------------------------------------------------
def norms(o, s):
    o, s = np.asarray(o, np.float64), np.asarray(s, np.float64)
    return (o * o).sum(-1) + DIVCONST, (s * s).sum(-1) + DIVCONST, (o * s).sum(-1) + DIVCONST


def cc(o, s):
    n_oo, n_ss, n_os = norms(o, s)
    return n_os / (np.sqrt(n_oo) * np.sqrt(n_ss))


def misfit(o, s, w=None):
    c = cc(o, s)
    w = np.ones_like(c) if w is None else np.asarray(w, np.float64)
    return 0.5 * (-2.0 * float((w * c).sum()))


def adjoint_source(o, s, w=None):
    """-d misfit / d s in conditioned data space"""
    o, s = np.asarray(o, np.float64), np.asarray(s, np.float64)
    n_oo, n_ss, n_os = norms(o, s)
    w = np.ones_like(n_oo) if w is None else np.asarray(w, np.float64)
    return (w / (np.sqrt(n_oo) * np.sqrt(n_ss)))[..., None] * (o - (n_os / n_ss)[..., None] * s)


# ---- the chain of a parameter file ----------------------------------------------------------------------------------------------------------
def weights_of(O, pb, sid):
    """w_r of one shot: float32 weights[r] and src_weight, multiplied in float64; ones without if_win"""
    cond = O.conditioning_of(pb["para"], pb["survey"], int(sid))
    n = int(pb["survey"]["shot%d" % int(sid)]["nrec"])
    if cond is None or cond["win"] is None:
        return np.ones(n)
    win = cond["win"]
    return np.asarray(win["weights"], np.float32)[:n].astype(np.float64) * float(np.float32(win["src_weight"]))


def data_misfit(O, pb, obs, syn):
    """per-shot raw gathers -> (misfit, [a per shot, float32 raw data space], sum_r |w_r| over the shots)"""
    total, adj, wsum = 0.0, [], 0.0
    for o, s, sid in zip(obs, syn, G.shots_of(pb)):
        co, cs, w = G.C_of(O, pb, o, sid), G.C_of(O, pb, s, sid), weights_of(O, pb, sid)
        total += misfit(co, cs, w)
        wsum += float(np.abs(w).sum())
        adj.append(G.Ct_of(O, pb, adjoint_source(co, cs, w).astype(np.float32), sid))
    return total, adj, wsum


def float32_restatement(O, pb, obs, syn):
    """the same through oracle.conditioned_residual, the float32 restatement that the suite's other cross-correlation tests compare with"""
    total, adj = 0.0, []
    for o, s, sid in zip(obs, syn, G.shots_of(pb)):
        obj, r, _, _ = O.conditioned_residual(o, s, float(pb["para"]["dt"]), O.conditioning_of(pb["para"], pb["survey"], int(sid)))
        total += obj
        adj.append(r)
    return 0.5 * total, adj


# ---- nearly fitting data ------------------------------------------------------------------------------------------------------------------------
def near_fit(syn, noise, c, eta):
    """obs = c syn + eta noise per shot, rounded once to float32 (the reference sees the rounded gathers)"""
    return [(c * s.astype(np.float64) + eta * n.astype(np.float64)).astype(np.float32) for s, n in zip(syn, noise)]
