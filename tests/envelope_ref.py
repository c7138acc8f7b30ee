"""The reference for the envelope misfit (parameter key if_envelope_misfit; include/sepfwi.h under sepfwi_cufd, sepfwi_data_misfit,
sepfwi_data_gn), outside the GPU: numpy, float64 on float32 inputs.

    H        the discrete Hilbert transform: zero-pad to 2 nt, real FFT (nt + 1 bins), bin k times -i for 0 < k < nt and times 0 for
             k = 0 and k = nt, inverse FFT (numpy scales by 1 / (2 nt)), crop to nt.  H^T = -H exactly.
    e(x)     x^2 + (H x)^2, the SQUARED envelope, pointwise
    misfit   1/2 |rho|^2,  rho = Z (e(o) - e(s)),  o = C obs, s = C syn, Z the zeroing of time sample 0
    D        de/ds = 2 [diag(s) + diag(H s) H],   D^T = 2 [diag(s) - H diag(H s)]
    a        the adjoint source the propagator injects, -d misfit / d syn = C^T D^T rho
    GN       C^T D^T Z D C, D at s

C and C^T are the oracle's cond_window / cond_bandpass composed as tests/cond_gn_ref.py composes them ("window, then band-pass" and
"band-pass, then window"); under the key ALONE C is the plain end taper, as for every live conditioning key (oracle.conditioning_of does
not know the key: cond_of adds that case).  Gradients of a reference-style pass come from oracle.cufd(calc_id=1, adj_src=a) with the
conditioning keys stripped -- the hook the oracle's own chain uses; J is tests/born_ref.py.  Nothing of the propagator is restated."""
import numpy as np

import cond_gn_ref as G
from fuzz_common import groups

KEY = "if_envelope_misfit"
STRIP = G.COND_KEYS + (KEY,)


# ---- the definitions, on (..., nt) arrays ----------------------------------------------------------------------------------------------
def hilbert(x, keep_nyquist=False):
    x = np.asarray(x, np.float64)
    nt = x.shape[-1]
    X = np.fft.rfft(x, n=2 * nt, axis=-1)
    m = np.full(nt + 1, -1j)
    m[0] = 0.0
    if not keep_nyquist:
        m[nt] = 0.0
    return np.fft.irfft(X * m, n=2 * nt, axis=-1)[..., :nt]


def env(x):
    x = np.asarray(x, np.float64)
    return x * x + hilbert(x) ** 2


def Z(d):
    out = np.array(d, np.float64, copy=True)
    out[..., 0] = 0.0
    return out


def rho(o, s):
    return Z(env(o) - env(s))


def misfit(o, s):
    r = rho(o, s)
    return 0.5 * float((r * r).sum())


def D(s, d):
    s, d = np.asarray(s, np.float64), np.asarray(d, np.float64)
    return 2.0 * (s * d + hilbert(s) * hilbert(d))


def Dt(s, w):
    s, w = np.asarray(s, np.float64), np.asarray(w, np.float64)
    return 2.0 * (s * w - hilbert(hilbert(s) * w))


def hilbert_term(s, w):
    """2 H((H s) w): the half of D^T w that a pass without the transform of the product would drop"""
    return 2.0 * hilbert(hilbert(np.asarray(s, np.float64)) * np.asarray(w, np.float64))


def adjoint_source(o, s):
    """D^T rho in conditioned data space: -d misfit / d s"""
    return Dt(s, rho(o, s))


def gn(s, d):
    """D^T Z D d"""
    return Dt(s, Z(D(s, d)))


# ---- the chain of a parameter file ----------------------------------------------------------------------------------------------------------
def cond_of(O, pb, sid):
    """oracle.conditioning_of without the key; the key alone: the end taper, no filter"""
    para = {k: v for k, v in pb["para"].items() if k != KEY}
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


def data_misfit(O, pb, obs, syn):
    """per-shot raw gathers -> (misfit, [a per shot, float32 raw data space], [rho], [D^T rho])"""
    total, adj, rhos, dts = 0.0, [], [], []
    for o, s, sid in zip(obs, syn, G.shots_of(pb)):
        co, cs = C_of(O, pb, o, sid), C_of(O, pb, s, sid)
        r = rho(co, cs)
        total += 0.5 * float((r * r).sum())
        w = Dt(cs, r)
        rhos.append(r)
        dts.append(w)
        adj.append(Ct_of(O, pb, w.astype(np.float32), sid))
    return total, adj, rhos, dts


def zdc(O, pb, syn, d):
    """Z D C d per shot (float64), D at C syn"""
    return [Z(D(C_of(O, pb, s, sid), C_of(O, pb, x, sid))) for s, x, sid in zip(syn, d, G.shots_of(pb))]


def data_gn(O, pb, syn, d):
    """C^T D^T Z D C d per shot, float32"""
    return [Ct_of(O, pb, Dt(C_of(O, pb, s, sid), q).astype(np.float32), sid) for s, q, sid in zip(syn, zdc(O, pb, syn, d), G.shots_of(pb))]


def plain_para(pb):
    return {k: v for k, v in pb["para"].items() if k not in STRIP}


def gradient(O, pb, adj, model="lame_init", gauge=0):
    """the oracle's backward pass with the adjoint source a (per shot (nrec, nSteps)) injected: dict(gLambda, gMu, gDen, gStf).  Shots
    with different channel counts run one at a time (fuzz_common.groups) and are summed in shot order; gauge = G cells: the channels are
    gauge channels, a is spread over their members (gauge_ref.inject)."""
    m = [t.numpy() for t in pb[model]]
    stf, ids = pb["Stf"].numpy(), pb["Shot_ids"].numpy()
    if gauge:
        import gauge_ref
        return gauge_ref.inject(O, m, stf, ids, plain_para(pb), pb["survey"], gauge, [np.asarray(x, np.float32) for x in adj])
    out, pos = None, 0
    for grp in groups(ids, pb["survey"]):
        a = np.ascontiguousarray(np.stack([np.asarray(x, np.float32) for x in adj[pos:pos + len(grp)]]))
        pos += len(grp)
        r = O.cufd(*m, stf, 1, np.asarray(grp, np.int32), plain_para(pb), pb["survey"], adj_src=a)
        if out is None:
            out = r
        else:
            for k in ("gLambda", "gMu", "gDen"):
                out[k] = out[k] + r[k]
            out["gStf"] = np.concatenate([out["gStf"], r["gStf"]], axis=0)
    return out


# ---- the problem of the GPU tests -----------------------------------------------------------------------------------------------------------
GPU_FILTER = [4.0, 8.0, 35.0, 50.0]      # problems.cond_problem's
KEYSETS = {"alone": {}, "filter": {"filter": GPU_FILTER}, "window": {"if_win": True}, "both": {"filter": GPU_FILTER, "if_win": True}}


def gpu_problem(tmp, keys, name=None, key=True, **more):
    """The problem of tests/test_gpu_envelope_misfit.py: problems.cond_problem's sizes (44 x 60, 300 steps, two shots) with its windows and
    weights in the survey, and a parameter file of its own (fuzz_common.write_para) that holds the key and the keys of KEYSETS[keys];
    key=False: the same file without the key."""
    import problems as P
    from fuzz_common import write_para
    pb = P.cond_problem(tmp, "window")
    base = dict(pb, para={k: v for k, v in pb["para"].items() if k not in STRIP})
    extra = dict(KEYSETS[keys], **more)
    if key:
        extra[KEY] = True
    fn, para = write_para(base, name or ("env_" + keys), **extra)
    return dict(pb, para_fname=fn, para=para, data_dir=para["data_dir_name"])


# ---- the synthetic traces of the issue's float64 check -------------------------------------------------------------------------------------------
def wavelet(nt=400, dt=1e-3, f=20.0, sigma=0.08, t0=0.15, shift=0.0):
    """a 20 Hz cosine under a Gaussian of 80 ms, centred at t0 + shift"""
    t = np.arange(nt) * dt - t0 - shift
    return np.cos(2.0 * np.pi * f * t) * np.exp(-0.5 * (t / sigma) ** 2)


def band_limited(rng, nrec, nt, lo=0.05, hi=0.35):
    """seeded random traces with their energy between lo and hi of the Nyquist frequency (float32); nt < 8: white.  Every trace has a
    peak of its own between 0.5 and 1.5 (two traces of two samples would else share the one sample that C leaves)."""
    x = rng.standard_normal((nrec, nt))
    if nt >= 8:
        X = np.fft.rfft(x, axis=1)
        k = np.arange(X.shape[1]) / max(X.shape[1] - 1, 1)
        X *= ((k >= lo) & (k <= hi))[None, :]
        x = np.fft.irfft(X, n=nt, axis=1)
    return (x / np.abs(x).max(axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (nrec, 1))).astype(np.float32)
