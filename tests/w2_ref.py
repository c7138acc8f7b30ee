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
tests/test_w2_reference.py licenses the hand gradient against autograd and central differences.

For the fuzz tests (tests/test_gpu_w2_kernel_fuzz.py, tests/test_gpu_w2_fuzz.py, tests/test_w2_fuzz_reference.py): trace_kinds, the seeded
traces that are not band-limited noise; tie_margin, by how much the reference decides its j(i); amplification, how far one float32
rounding of the synthetic gathers moves the result; and the deliberate errors of trace_parts / conditioned_misfit that show that the
comparisons can fail."""
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


def trace_parts(o, s, dt, beta=BETA, scale_from=None, tile=None, project=True):
    """one trace -> dict(W, dWds (n,), T, j, F, Gc, f, g, psi, c) in float64; None for a dead trace.  scale_from: the trace A is taken
    from (the observed one; tests/test_w2_reference.py passes the synthetic one as a deliberate error).  Two more deliberate errors for
    tests/test_w2_fuzz_reference.py: tile, the suffix sums of c start again every `tile` samples counted from the trace's end (a block
    scan that drops its carry); project=False, psi without its mean under f."""
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
    suffix = np.cumsum(c[::-1])
    if tile:
        lead = np.arange(suffix.size) // tile * tile      # the first sample (from the end) of each tile
        suffix = suffix - np.where(lead > 0, suffix[np.maximum(lead - 1, 0)], 0.0)
    psi = d + suffix[::-1]
    dq = (psi - ((f * psi).sum() if project else 0.0)) / Ss
    dWds = np.zeros(n)
    dWds[1:] = sigmoid(beta * s[1:] / A) * (beta / A) * dq
    return dict(W=W, dWds=dWds, T=T, j=j, F=F, Gc=Gc, f=f, g=g, psi=psi, c=c, d=d, Ss=Ss, A=A)


def trace_weights(win, nrec):
    """w_r: weights[r] * src_weight as a float32 product under if_win (win: the oracle's window dict), else 1"""
    if win is None:
        return np.ones(nrec)
    return (np.asarray(win["weights"], np.float32) * np.float32(win["src_weight"])).astype(np.float64)


def gather(o, s, dt, beta=BETA, w=None, **wrong):
    """conditioned gathers (nrec, n) -> (sum_r w_r W_r, a (nrec, n) float64, W per trace); wrong: trace_parts' deliberate errors
    (scale_from="syn": A from the synthetic trace)"""
    o, s = np.asarray(o), np.asarray(s)
    nrec = o.shape[0]
    w = np.ones(nrec) if w is None else np.asarray(w, np.float64)
    a, Ws = np.zeros(o.shape), np.zeros(nrec)
    for r in range(nrec):
        p = trace_parts(o[r], s[r], dt, beta, **dict(wrong, scale_from=s[r]) if wrong.get("scale_from") == "syn" else wrong)
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


def conditioned_misfit(O, pb, cobs, csyn, beta=None, first_weight=False, **wrong):
    """per-shot CONDITIONED gathers -> (misfit, [a per shot in conditioned data space, float64], [W per trace]).  Deliberate errors for
    tests/test_w2_fuzz_reference.py: beta, another one than the file's; first_weight, w_0 for every channel; wrong: gather's"""
    total, adj, Ws = 0.0, [], []
    for o, s, sid in zip(cobs, csyn, G.shots_of(pb)):
        cond = cond_of(O, pb, sid)
        w = trace_weights(cond["win"] if cond else None, np.asarray(o).shape[0])
        if first_weight:
            w = np.full_like(w, w[0])
        tot, a, W = gather(o, s, float(pb["para"]["dt"]), beta_of(pb) if beta is None else beta, w, **wrong)
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


# ---- the trace kinds of tests/test_gpu_w2_kernel_fuzz.py ---------------------------------------------------------------------------------
KINDS = ("band-limited pair", "late arrival after exact zeros", "syn 1e3 x", "syn 1e-3 x", "syn all zeros", "one-signed", "spiked obs")
SHIFT = 3             # the whole-sample delay of the eighth kind
KIND_SEED0 = 4100     # offset of the kinds' generator (tests/test_w2_fuzz_reference.py: every case meets the tie-margin condition)


def arrival(nt, onset, centre, width):
    """a Ricker arrival centred at sample `centre` of half-width `width` samples, EXACT zeros before sample `onset`"""
    i = np.arange(nt, dtype=np.float64)
    x = (np.pi * (i - centre) / width) ** 2
    out = (1.0 - 2.0 * x) * np.exp(-x)
    out[:int(onset)] = 0.0
    return out


def trace_kinds(nt, seed):
    """The seeded traces of the kernel fuzz, float32: -> dict(obs (7, nt), syn (7, nt): one channel per kind of KINDS;
    shift_obs, shift_syn (7, nt): the eighth kind on every channel, syn the observed trace delayed by SHIFT whole samples, exact zeros
    over the first and the last SHIFT + 1 samples of both)."""
    rng = np.random.default_rng(KIND_SEED0 + seed)
    b = E.band_limited(rng, 12, nt).astype(np.float64)
    obs, syn = np.zeros((7, nt)), np.zeros((7, nt))
    obs[0], syn[0] = b[0], b[1]
    amp = rng.uniform(0.5, 1.5, 2)
    obs[1] = amp[0] * arrival(nt, int(0.6 * nt), 0.78 * nt, 0.09 * nt)
    syn[1] = amp[1] * arrival(nt, int(0.3 * nt), 0.48 * nt, 0.09 * nt)
    obs[2], syn[2] = b[2], 1e3 * b[3]
    obs[3], syn[3] = b[4], 1e-3 * b[5]
    obs[4] = b[6]
    obs[5], syn[5] = -np.abs(b[7]), np.abs(b[8])
    obs[6], syn[6] = b[9], b[10]
    at = int(rng.integers(nt // 4, 3 * nt // 4))
    obs[6, at] = 100.0 * np.abs(b[9]).max() * (1.0 if b[9, at] >= 0 else -1.0)
    so = E.band_limited(rng, 7, nt).astype(np.float64)
    so[:, :SHIFT + 1] = 0.0
    so[:, nt - SHIFT - 1:] = 0.0
    ss = np.zeros_like(so)
    ss[:, SHIFT:] = so[:, :nt - SHIFT]
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    return dict(obs=f32(obs), syn=f32(syn), shift_obs=f32(so), shift_syn=f32(ss))


def tie_margin(o, s, dt, beta=BETA):
    """one trace -> the smallest of |F_i - G_j(i)| and |F_i - G_(j(i)-1)| over the samples i, a node counted only where the search
    compares F_i with it: not node 0 (the search starts at j = 1) and not node n - 1 (the clamp).  j(i) is decided by a margin that a
    float64 summation in another order cannot move where this is far above n 2^-53.  inf for a dead trace."""
    p = trace_parts(o, s, dt, beta)
    if p is None:
        return np.inf
    n = np.asarray(o).shape[0]
    F, Gc, j = p["F"], p["Gc"], p["j"]
    up = np.where(j < n - 1, np.abs(F - Gc[j]), np.inf)
    down = np.where(j - 1 > 0, np.abs(F - Gc[j - 1]), np.inf)
    return float(min(up.min(), down.min())) if F.size else np.inf


def amplification(pb, obs, syn, seeds=(0, 1, 2), O=None):
    """How far one float32 rounding of the synthetic gathers moves the result, by the reference's own measure: every sample of syn times
    (1 + e 2^-24), e random signs, in float64 (C is linear: C syn + 2^-24 C (e . syn), C the plain oracle build's) -> (kappa_a, kappa_W),
    the largest movements over the seeds of C^T a in rel-L2 and of the misfit in relative terms, divided by 2^-24."""
    if O is None:
        from oracle import oracle as O
    eta = 2.0 ** -24
    ids = G.shots_of(pb)
    co = [C_of(O, pb, o, sid) for o, sid in zip(obs, ids)]
    cs = [C_of(O, pb, s, sid).astype(np.float64) for s, sid in zip(syn, ids)]
    f0, a0, _ = conditioned_misfit(O, pb, co, cs)

    def ct(a):      # C^T in float32 on arrays scaled to order 1 (linear: the scale comes back afterwards)
        k = max(float(np.abs(x).max()) for x in a) or 1.0
        return [k * Ct_of(O, pb, (x / k).astype(np.float32), sid).astype(np.float64) for x, sid in zip(a, ids)]

    n0 = G.norm(ct(a0))
    ka = kw = 0.0
    for seed in seeds:
        rng = np.random.default_rng([7919, seed])
        e = [rng.integers(0, 2, np.shape(s)).astype(np.float32) * 2 - 1 for s in syn]
        dcs = [C_of(O, pb, np.asarray(s, np.float32) * x, sid).astype(np.float64) for s, x, sid in zip(syn, e, ids)]
        f1, a1, _ = conditioned_misfit(O, pb, co, [c + eta * d for c, d in zip(cs, dcs)])
        da = ct([x - y for x, y in zip(a1, a0)])
        ka = max(ka, G.norm(da) / max(n0, 1e-300) / eta)
        kw = max(kw, abs(f1 - f0) / max(abs(f0), 1e-300) / eta)
    return ka, kw


# ---- the cases of tests/test_gpu_w2_kernel_fuzz.py (tests/test_w2_fuzz_reference.py checks their tie margins on the CPU) ---------------
FUZZ_BETAS = (0.25, 1.0, 8.0, 16.0)      # 3.0 is held by tests/test_gpu_w2_data.py
FUZZ_NTS = (66, 257, 258, 1025)          # the mass samples nt - 1 on both sides of a wave (64) and of a tile (256), and a fourth tile's carry
TIE_FACTOR = 64.0                        # a live trace's tie margin is at least this times nt 2^-53


def kind_seed(nt, beta):
    """the seed of trace_kinds for a case: one per (nt, beta), shared by the key sets"""
    return 10 * FUZZ_NTS.index(nt) + FUZZ_BETAS.index(beta)
