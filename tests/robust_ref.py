"""The reference for the robust misfits (parameter keys robust_misfit / robust_delta / robust_quantile; csrc/robust_misfit.hpp and
include/sepfwi.h under sepfwi_cufd), outside the GPU: numpy, float64 on float32 inputs.

Per trace of nt samples, o = C obs and s = C syn; the live samples are i = 1 ... nt - 1 (sample 0 is zeroed: the project's Z):

    A        np.sort(np.abs(o[1:]))[k], k = floor(q (n - 1)), n = nt - 1: no interpolation, a float32 value.  A == 0: a dead trace,
             misfit 0, adjoint source 0, weight 0
    delta    robust_delta A;  r = o - s;  u = r / delta
    huber    phi = delta^2 u^2 / 2 for |u| <= 1, else delta^2 (|u| - 1/2);  w = min(1, 1 / |u|)
    cauchy   phi = delta^2 / 2 log1p(u^2);  w = 1 / (1 + u^2)
    misfit   sum_traces sum_i phi (the library accumulates 2 sum phi and halves the total)
    a        -d misfit / d s = psi = r w,  a_0 = 0
    GN       d -> Z diag(w) Z d with w at (o, background s): the IRLS weight

C and C^T are the oracle's cond_window / cond_bandpass as tests/w2_ref.py composes them; under the key ALONE C is the plain end taper, as
for every live conditioning key.  tests/test_robust_reference.py licenses psi against autograd and central differences."""
import numpy as np

import cond_gn_ref as G
import envelope_ref as E

KEY, DELTA_KEY, Q_KEY = "robust_misfit", "robust_delta", "robust_quantile"
KEYS = (KEY, DELTA_KEY, Q_KEY)
QUANTILE = 0.9
KINDS = ("huber", "cauchy")
STRIP = E.STRIP + KEYS


def rank(n, q):
    """k of the definition for n live samples"""
    return min(max(int(np.floor(q * (n - 1))), 0), n - 1)


def scale(o, q=QUANTILE):
    """A of one trace: the order statistic of |o[1:]|, as a float (the float32 value, exactly); 0 for a trace without a live sample"""
    v = np.sort(np.abs(np.asarray(o)[1:]))
    return float(v[rank(v.size, q)]) if v.size else 0.0


def trace_parts(o, s, kind, delta, q=QUANTILE, scale_from=None):
    """one trace -> dict(A, phi (sum), psi (nt,), w (nt,; 0 at sample 0)) in float64; zeros for a dead trace.  scale_from: the trace A is
    taken from (the observed one; tests/test_robust_reference.py passes the synthetic one as a deliberate error)"""
    assert kind in KINDS
    o64, s64 = np.asarray(o, np.float64), np.asarray(s, np.float64)
    nt = o64.shape[0]
    A = scale(o if scale_from is None else scale_from, q)
    psi, w = np.zeros(nt), np.zeros(nt)
    if A == 0.0:
        return dict(A=0.0, phi=0.0, psi=psi, w=w)
    d = float(delta) * A
    r = o64[1:] - s64[1:]
    u = r / d
    au = np.abs(u)
    if kind == "huber":
        inside = au <= 1.0
        phi = np.where(inside, d * d * (0.5 * u * u), d * d * (au - 0.5))
        w[1:] = np.where(inside, 1.0, 1.0 / np.maximum(au, 1.0))
    else:
        phi = 0.5 * d * d * np.log1p(u * u)
        w[1:] = 1.0 / (1.0 + u * u)
    psi[1:] = r * w[1:]
    return dict(A=A, phi=float(phi.sum()), psi=psi, w=w)


def gather(o, s, kind, delta, q=QUANTILE):
    """conditioned gathers (nrec, nt) -> (sum phi, psi (nrec, nt) float64, w (nrec, nt) float64, A per trace)"""
    o, s = np.asarray(o), np.asarray(s)
    psi, w, A, tot = np.zeros(o.shape), np.zeros(o.shape), np.zeros(o.shape[0]), 0.0
    for r in range(o.shape[0]):
        p = trace_parts(o[r], s[r], kind, delta, q)
        psi[r], w[r], A[r] = p["psi"], p["w"], p["A"]
        tot += p["phi"]
    return tot, psi, w, A


# ---- the chain of a parameter file -----------------------------------------------------------------------------------------------------
def cond_of(O, pb, sid):
    """oracle.conditioning_of without the keys; the key alone: the end taper, no filter"""
    para = {k: v for k, v in pb["para"].items() if k not in KEYS}
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


def keys_of(pb):
    return pb["para"][KEY], float(pb["para"][DELTA_KEY]), float(pb["para"].get(Q_KEY, QUANTILE))


def conditioned_misfit(pb, cobs, csyn):
    """per-shot CONDITIONED gathers -> (misfit, [psi per shot, float64], [w per shot, float64], [A per trace])"""
    kind, delta, q = keys_of(pb)
    total, adj, ws, As = 0.0, [], [], []
    for o, s in zip(cobs, csyn):
        tot, psi, w, A = gather(o, s, kind, delta, q)
        total += tot
        adj.append(psi)
        ws.append(w)
        As.append(A)
    return total, adj, ws, As


def conditioned_gn(pb, cobs, csyn, cd):
    """per-shot CONDITIONED gathers -> [Z w Z d per shot, float64], w at (cobs, csyn)"""
    _, _, ws, _ = conditioned_misfit(pb, cobs, csyn)
    return [w * np.asarray(d, np.float64) for w, d in zip(ws, cd)]


def data_misfit(O, pb, obs, syn):
    """per-shot raw gathers -> (misfit, [a per shot, float32 raw data space], [psi before C^T, float64]); C and C^T the oracle's"""
    ids = G.shots_of(pb)
    cobs = [C_of(O, pb, o, sid) for o, sid in zip(obs, ids)]
    csyn = [C_of(O, pb, s, sid) for s, sid in zip(syn, ids)]
    total, adj, _, _ = conditioned_misfit(pb, cobs, csyn)
    return total, [Ct_of(O, pb, a.astype(np.float32), sid) for a, sid in zip(adj, ids)], adj


def data_gn(O, pb, obs, syn, d):
    """per-shot raw gathers -> [C^T Z W Z C d per shot, float32]"""
    ids = G.shots_of(pb)
    c = lambda gs: [C_of(O, pb, g, sid) for g, sid in zip(gs, ids)]
    out = conditioned_gn(pb, c(obs), c(syn), c(d))
    return [Ct_of(O, pb, x.astype(np.float32), sid) for x, sid in zip(out, ids)]


def add_spikes(o, m, rng, q=QUANTILE, factor=100.0):
    """a copy of the gather o (nrec, nt) with m spikes of +-factor x the trace's peak in every live trace -> (copy, [indices per trace]).
    The spikes replace samples whose |o| is ABOVE A (there are n - 1 - k of them without ties, so m < (1 - q) n fit): the samples up to rank
    k stay what they were and A keeps its bits.  (A spike on a sample below rank k would move the order statistic up one rank, to the next
    larger |o|: a second, small effect that the tests of the scale cover on their own.)"""
    out, where = np.array(o, np.float32), []
    for r in range(out.shape[0]):
        above = 1 + np.flatnonzero(np.abs(out[r, 1:]) > scale(out[r], q))
        if above.size < m:      # a dead or constant trace
            where.append(np.zeros(0, int))
            continue
        idx = rng.choice(above, size=m, replace=False)
        peak = np.abs(out[r]).max()
        out[r, idx] = (np.float32(factor) * peak * rng.choice([-1.0, 1.0], size=m)).astype(np.float32)
        where.append(idx)
    return out, where


def spike_plan(co, seed, q=QUANTILE, m=5):
    """Where add_spikes' spikes go when the misfit sees the gather through a chain C: co = C obs of ONE build (nrec, nt) -> [indices per
    trace] and [signs per trace].  The samples are chosen on |C obs|, so inside the trace's window (outside it C obs is 0, never above
    A): m samples above A where there are m, ONE where there are fewer -- a sample above A if there is one, else the trace's largest
    (q = 1.0: A is the maximum and nothing lies above it) -- and none on a dead trace (A == 0).  seed: a sequence of integers; every
    trace has a generator of its own, default_rng(seed + [trace]), so that one trace never shifts another's."""
    where, signs = [], []
    for r in range(co.shape[0]):
        rng = np.random.default_rng(list(seed) + [r])
        A = scale(co[r], q)
        a = np.abs(np.asarray(co[r], np.float64)[1:])
        above = 1 + np.flatnonzero(a > A)
        if A == 0.0:
            idx = np.zeros(0, int)
        elif above.size >= m:
            idx = np.sort(rng.choice(above, size=m, replace=False))
        elif above.size:
            idx = rng.choice(above, size=1)
        else:
            idx = np.array([1 + int(np.argmax(a))])
        where.append(idx)
        signs.append(rng.choice([-1.0, 1.0], size=idx.size))
    return where, signs


def put_spikes(o, where, signs, factor=100.0):
    """a copy of the RAW gather o with +-factor x each trace's own peak at the planned samples (spike_plan): the other oracle build's
    gather gets its spikes at the same samples with its own peak.

    What this does to A.  Under the key alone C is the end taper (1 except over the record's last samples) and under if_win without a
    filter it is a gain per sample: a sample that was above A stays above it (its |C obs| only grew), the samples up to rank k stay
    what they were and A KEEPS ITS BITS -- as add_spikes on the raw gather under the key alone.  Two exceptions.  At q = 1.0 the one
    spike replaces the maximum, so A becomes the spike's own value, 100 x the trace's peak through C, on both builds alike.  Under a
    filter a spike is spread over the record by the band-pass, A is the order statistic of the filtered spiked trace and has nothing
    in common with the clean trace's; it is still the same functional of the same installed gather for the library and for the
    reference, and the two builds' A differ by what their band-passes differ by (fuzz_sides.robust_oracle_side holds that as a
    yardstick)."""
    out = np.array(o, np.float32)
    for r, (idx, sg) in enumerate(zip(where, signs)):
        if idx.size:
            out[r, idx] = (np.float32(factor) * np.abs(out[r]).max() * sg).astype(np.float32)
    return out
