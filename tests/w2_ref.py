"""The reference for the trace-wise quadratic Wasserstein (W2) misfit (parameter keys if_w2_misfit / w2_beta; include/sepfwi.h under
sepfwi_cufd and sepfwi_data_misfit), outside the GPU: numpy, float64 on float32 inputs.

Per trace, o = C obs and s = C syn with n samples, dt the float32 step, t_i = i dt, i = 1 ... n - 1 (sample 0 carries no mass: the
project's Z; it is the CDF's node with value 0 at t_0):

    A        max |o| over the whole trace; A == 0: a dead trace, misfit 0 and adjoint source 0
    q(x)     softplus(beta x / A) = max(z, 0) + log1p(exp(-|z|));  qs = q(s), qo = q(o)
    f, g     qs / sum qs,  qo / sum qo
    F, G     the prefix sums of qs (qo), each divided by its own last entry; G_0 = 0
    j(i)     the first j >= 1 with G_j >= F_i, clamped to n - 1
    T_i      t_{j-1} + dt (F_i - G_{j-1}) / g_j         (the linear interpolation of the inverse of G)
    W        sum_i f_i (t_i - T_i)^2
    misfit   1/2 sum_r w_r W_r,  w_r = weights[r] * src_weight (a float32 product) under if_win, else 1
    a        -d misfit / d s:  c_i = 2 f_i (T_i - t_i) dt / g_j(i),  psi_k = (t_k - T_k)^2 + sum_{i >= k} c_i,
             dW/dqs_k = (psi_k - sum_l f_l psi_l) / sum qs,  dW/ds_k = sigmoid(beta s_k / A) (beta / A) dW/dqs_k,
             a_0 = 0, a_k = -1/2 w_r dW/ds_k

C and C^T are the oracle's cond_window / cond_bandpass as tests/envelope_ref.py composes them; under the key ALONE C is the plain end
taper, as for every live conditioning key (oracle.conditioning_of does not know the key: cond_of adds that case).
tests/test_w2_reference.py licenses the hand gradient against autograd and central differences."""
import numpy as np

import cond_gn_ref as G
import envelope_ref as E

KEY = "if_w2_misfit"
BETA_KEY = "w2_beta"
BETA = 3.0
STRIP = E.STRIP + (KEY, BETA_KEY)


def softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def sigmoid(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def trace_parts(o, s, dt, beta=BETA, scale_from=None):
    """one trace -> dict(W, dWds (n,), T, j, F, Gc, f, g, psi, c) in float64; None for a dead trace.  scale_from: the trace A is taken
    from (the observed one; tests/test_w2_reference.py passes the synthetic one as a deliberate error)"""
    o, s = np.asarray(o, np.float64), np.asarray(s, np.float64)
    n = o.shape[0]
    dt = float(np.float32(dt))
    A = float(np.abs(o if scale_from is None else np.asarray(scale_from, np.float64)).max())
    if A == 0.0:
        return None
    qs, qo = softplus(beta * s[1:] / A), softplus(beta * o[1:] / A)
    ps, po = np.cumsum(qs), np.cumsum(qo)
    Ss, So = ps[-1], po[-1]
    f, g = qs / Ss, qo / So
    F = ps / Ss
    Gc = np.concatenate([[0.0], po / So])                      # node l of G at index l, l = 0 ... n - 1
    j = np.minimum(np.searchsorted(Gc[1:], F, side="left") + 1, n - 1)
    t = np.arange(1, n) * dt
    T = (j - 1) * dt + dt * (F - Gc[j - 1]) / g[j - 1]
    d = (t - T) ** 2
    W = float((f * d).sum())
    c = 2.0 * f * (T - t) * dt / g[j - 1]
    psi = d + np.cumsum(c[::-1])[::-1]
    dq = (psi - (f * psi).sum()) / Ss
    dWds = np.zeros(n)
    dWds[1:] = sigmoid(beta * s[1:] / A) * (beta / A) * dq
    return dict(W=W, dWds=dWds, T=T, j=j, F=F, Gc=Gc, f=f, g=g, psi=psi, c=c, d=d, Ss=Ss, A=A)


def trace_weights(win, nrec):
    """w_r: weights[r] * src_weight as a float32 product under if_win (win: the oracle's window dict), else 1"""
    if win is None:
        return np.ones(nrec)
    return (np.asarray(win["weights"], np.float32) * np.float32(win["src_weight"])).astype(np.float64)


def gather(o, s, dt, beta=BETA, w=None):
    """conditioned gathers (nrec, n) -> (sum_r w_r W_r, a (nrec, n) float64, W per trace)"""
    o, s = np.asarray(o), np.asarray(s)
    nrec = o.shape[0]
    w = np.ones(nrec) if w is None else np.asarray(w, np.float64)
    a, Ws = np.zeros(o.shape), np.zeros(nrec)
    for r in range(nrec):
        p = trace_parts(o[r], s[r], dt, beta)
        if p is not None:
            Ws[r] = p["W"]
            a[r] = -0.5 * w[r] * p["dWds"]
    return float((w * Ws).sum()), a, Ws


# ---- the chain of a parameter file -----------------------------------------------------------------------------------------------------
def cond_of(O, pb, sid):
    """oracle.conditioning_of without the keys; the key alone: the end taper, no filter"""
    para = {k: v for k, v in pb["para"].items() if k not in (KEY, BETA_KEY)}
    c = O.conditioning_of(para, pb["survey"], int(sid))
    if c is None and pb["para"].get(KEY):
        c = dict(win=None, filter=None)
    return c


def C_of(O, pb, d, sid):
    cond = cond_of(O, pb, sid)
    d = np.asarray(d, np.float32)
    if cond is None:
        return d.copy()
    out = O.cond_window(d, float(pb["para"]["dt"]), cond["win"])
    if cond.get("filter") is not None:
        out = O.cond_bandpass(out, float(pb["para"]["dt"]), cond["filter"])
    return out


def Ct_of(O, pb, d, sid):
    cond = cond_of(O, pb, sid)
    out = np.asarray(d, np.float32)
    if cond is None:
        return out.copy()
    if cond.get("filter") is not None:
        out = O.cond_bandpass(out, float(pb["para"]["dt"]), cond["filter"])
    return O.cond_window(out, float(pb["para"]["dt"]), cond["win"])


def beta_of(pb):
    return float(pb["para"].get(BETA_KEY, BETA))


def conditioned_misfit(O, pb, cobs, csyn):
    """per-shot CONDITIONED gathers -> (misfit, [a per shot in conditioned data space, float64], [W per trace])"""
    total, adj, Ws = 0.0, [], []
    for o, s, sid in zip(cobs, csyn, G.shots_of(pb)):
        cond = cond_of(O, pb, sid)
        w = trace_weights(cond["win"] if cond else None, np.asarray(o).shape[0])
        tot, a, W = gather(o, s, float(pb["para"]["dt"]), beta_of(pb), w)
        total += 0.5 * tot
        adj.append(a)
        Ws.append(W)
    return total, adj, Ws


def data_misfit(O, pb, obs, syn):
    """per-shot raw gathers -> (misfit, [a per shot, float32 raw data space], [a before C^T, float64]); C and C^T the oracle's"""
    cobs = [C_of(O, pb, o, sid) for o, sid in zip(obs, G.shots_of(pb))]
    csyn = [C_of(O, pb, s, sid) for s, sid in zip(syn, G.shots_of(pb))]
    total, adj, _ = conditioned_misfit(O, pb, cobs, csyn)
    return total, [Ct_of(O, pb, a.astype(np.float32), sid) for a, sid in zip(adj, G.shots_of(pb))], adj


# ---- the synthetic traces of the issue's float64 checks ----------------------------------------------------------------------------------
def ricker_pair(nt=600, dt=1e-3, f=15.0, t0=(0.20, 0.32), amp=(1.0, -0.6), shift=0.0):
    """a two-arrival Ricker trace of peak frequency f, the arrivals at t0 + shift"""
    t = np.arange(nt) * dt
    out = np.zeros(nt)
    for tc, a in zip(t0, amp):
        x = (np.pi * f * (t - tc - shift)) ** 2
        out += a * (1.0 - 2.0 * x) * np.exp(-x)
    return out
