"""The reference of the apparent-slowness (f-k) fan filter of the conditioning chain (parameter keys fk_slowness / fk_mode; csrc/conditioning.hpp:
fk_filter), outside the GPU: numpy float64 of the definition through the FULL complex fft2 -- no half spectrum, no transposition, nothing of
the device's arrangement.  tests/test_fk_reference.py licenses it (real output, symmetric operator, reject = 1 - pass, the two-plane-wave
gather, the Nyquist rule).

The stage, on one shot's (nrec, nt) gather d sampled at dt with the channel spacing delta along the fibre:
    zero-pad to (P, 2 nt), P the smallest power of two >= 2 nrec; forward DFT along both axes (e^{-i...});
    bin (m, j): k_m = m / (P delta) for m <= P / 2 else (m - P) / (P delta), f_j likewise with 2 nt and dt; slowness p = -k / f (p > 0: an
    event that arrives later at higher channel indices); at f = 0: p = 0 for k = 0, infinite (T = 0) otherwise;
    T(p) = 0 outside (p1, p4), 1 on [p2, p3], sin^2 / cos^2 ramps between; G = T (pass) or 1 - T (reject); on the time-Nyquist bins j = nt and the
    wavenumber-Nyquist bins m = P / 2 the gain uses (T(p) + T(-p)) / 2 in place of T(p);
    multiply, inverse transforms (1 / (2 nt P)), crop to (nrec, nt).
The chain: C = FK . B . Wn (window, band-pass, fan), C^T = Wn . B . FK; the first two are the oracle's own (tests/cond_gn_ref.py), and like
every live conditioning key fk_slowness alone switches the window stage to its plain end taper."""
import numpy as np

import cond_gn_ref as G

SIZES = ((2, 2), (3, 3), (5, 64), (33, 65), (64, 257), (65, 600))      # (nrec, nt)
KEYS = ("fk_slowness", "fk_mode")


def padded(nrec):
    P = 1
    while P < 2 * nrec:
        P *= 2
    return P


def trapezoid(p, corners):
    p1, p2, p3, p4 = [float(v) for v in corners]
    p = np.asarray(p, np.float64)
    out = np.zeros_like(p)
    with np.errstate(invalid="ignore"):
        up = (p > p1) & (p < p2)
        out[up] = np.sin(0.5 * np.pi * (p[up] - p1) / (p2 - p1)) ** 2
        out[(p >= p2) & (p <= p3) & (p > p1) & (p < p4)] = 1.0
        down = (p > p3) & (p < p4)
        out[down] = np.cos(0.5 * np.pi * (p[down] - p3) / (p4 - p3)) ** 2
    return out


def gain(nt, P, dt, delta, corners, reject=False, nyquist=True):
    """G on the full (P, 2 nt) grid of bins; nyquist=False: the deliberately wrong variant without the Nyquist rule"""
    N = 2 * nt
    k = np.fft.fftfreq(P, delta)[:, None] * np.ones((1, N))
    f = np.ones((P, 1)) * np.fft.fftfreq(N, dt)[None, :]
    k[P // 2, :] = 0.5 / delta                                  # m = P / 2 counts as m <= P / 2: k = +1 / (2 delta) (fftfreq says -)
    f[:, nt] = 0.5 / dt                                         # ... and j = nt as +1 / (2 dt); the Nyquist rule makes the sign immaterial
    with np.errstate(divide="ignore", invalid="ignore"):
        p = -k / f
    p[(f == 0) & (k == 0)] = 0.0
    p[(f == 0) & (k != 0)] = np.inf
    T = trapezoid(p, corners)
    if nyquist:
        m = np.arange(P)[:, None] * np.ones((1, N), int)
        j = np.ones((P, 1), int) * np.arange(N)[None, :]
        T = np.where((j == nt) | (m == P // 2), 0.5 * (T + trapezoid(-p, corners)), T)
    return 1.0 - T if reject else T


def fk_full(d, dt, delta, corners, reject=False, nyquist=True):
    """-> (the real part of the full complex inverse, cropped, float64; max |imaginary part| / max |real part| over the WHOLE padded array)"""
    d = np.asarray(d, np.float64)
    nrec, nt = d.shape
    P = padded(nrec)
    x = np.zeros((P, 2 * nt))
    x[:nrec, :nt] = d
    y = np.fft.ifft2(np.fft.fft2(x) * gain(nt, P, float(dt), float(delta), corners, reject, nyquist))
    return y.real[:nrec, :nt].copy(), float(np.abs(y.imag).max() / max(np.abs(y.real).max(), 1e-300))


def fk(d, dt, delta, corners, reject=False):
    return fk_full(d, dt, delta, corners, reject)[0]


def spacing(para, survey, sid):
    """The channel spacing of one shot as the library derives it (csrc/host_checks.hpp: fk_channel_spacing); ValueError where it refuses"""
    sh = survey["shot%d" % int(sid)]
    n = int(sh["nrec"])
    z, x = np.asarray(sh["z_rec"][:n], np.int64), np.asarray(sh["x_rec"][:n], np.int64)
    if n == 0:
        return 0.0
    if n == 1:
        raise ValueError("fk_slowness: shot %d has exactly one channel" % sid)
    sz, sx = np.diff(z), np.diff(x)
    if sz[0] == 0 and sx[0] == 0:
        raise ValueError("fk_slowness: shot %d: a zero step" % sid)
    if (sz != sz[0]).any() or (sx != sx[0]).any():
        raise ValueError("fk_slowness: shot %d: the step is not constant" % sid)
    return float(np.hypot(float(sz[0]) * float(para["dz"]), float(sx[0]) * float(para["dx"])))


def _stage(pb, d, sid):
    para = pb["para"]
    return fk(d, float(para["dt"]), spacing(para, pb["survey"], sid), para["fk_slowness"], para.get("fk_mode", "pass") == "reject")      # float64, unrounded


def C_of(O, pb, d, sid):
    """C = FK . B . Wn on one shot's (nrec, nSteps) gather: cond_gn_ref.C_of (oracle.cond_window, oracle.cond_bandpass), then the stage above;
    under fk_slowness alone the window stage is the plain end taper.  Without the key: cond_gn_ref.C_of."""
    if pb["para"].get("fk_slowness") is None:
        return G.C_of(O, pb, d, sid)
    if O.conditioning_of(pb["para"], pb["survey"], int(sid)) is None:
        out = O.cond_window(np.asarray(d, np.float32), float(pb["para"]["dt"]), None)
    else:
        out = G.C_of(O, pb, d, sid)
    return _stage(pb, out, sid)


def Ct_of(O, pb, d, sid):
    """C^T = Wn . B . FK"""
    if pb["para"].get("fk_slowness") is None:
        return G.Ct_of(O, pb, d, sid)
    out = _stage(pb, d, sid)
    if O.conditioning_of(pb["para"], pb["survey"], int(sid)) is None:
        return O.cond_window(out, float(pb["para"]["dt"]), None)
    return G.Ct_of(O, pb, out, sid)


def without_fk(pb, name="nofk"):
    """pb's file pair without the fk keys, written next to it (a session of its own) -> a shallow copy of pb"""
    para = {k: v for k, v in pb["para"].items() if k not in KEYS}
    out = dict(pb)
    out["para_fname"], out["para"] = G.write_files(pb, name, para, pb["survey"])
    return out


def plane_waves(nrec=64, nt=400, dt=1e-3, delta=10.0, p0=4e-4, f0=25.0):
    """two Ricker plane waves of apparent slowness +p0 and -p0 -> (the +p0 event, the -p0 event), each (nrec, nt)"""
    t, x = np.arange(nt) * dt, np.arange(nrec) * delta

    def ricker(tt):
        a = (np.pi * f0 * tt) ** 2
        return (1.0 - 2.0 * a) * np.exp(-a)
    return ricker(t[None, :] - 0.06 - p0 * x[:, None]), ricker(t[None, :] - 0.06 - p0 * (x[-1] - x[:, None]))


# The pass-level problem (tests/test_gpu_fk_passes.py; its inputs are checked in tests/test_fk_reference.py): cond_gn_ref.SMALL in mode "both"
# plus the fan.  The fibre lies 320 m below the sources at x = 60 m and 410 m, so the direct wave crosses the 40 channels (spacing 10 m) with
# apparent slownesses from 0 below the source to about +-2.4e-4 s/m at the far end (sin(theta) / vp, vp about 3200 m/s): positive on most of
# shot 0, negative on most of shot 1.  The lower ramp 0.5e-4 ... 1.5e-4 cuts through shot 0's direct wave, and the band rejects shot 1's.
PASS_CORNERS = [0.5e-4, 1.5e-4, 6.0e-4, 8.0e-4]


def pass_problem(tmp, **keys):
    import problems as P
    return G.set_mode(P.make_problem(str(tmp), **G.SMALL), "both", name="fk_both", fk_slowness=PASS_CORNERS, **keys)
