"""The robust misfits' kernel alone, on the GPU (-m gpu), with no time loop: sepfwi_data_misfit and sepfwi_data_gn_obs through
fwi_ops.data_misfit / data_gn(obs=) under robust_misfit, against tests/robust_ref.py (float64 on float32 inputs;
tests/test_robust_reference.py licenses it).

Shapes: nSteps 2 (one live sample), 3, 64, 65, 257 and 1025 (past four strides of the block's 256 threads); one channel, five channels, and
two shots with 5 and 3.  Key sets: the key alone (C: the end taper), with filter, with if_win (channel 1 has weight 0: a dead trace; the
last channel of a shot with three or more an empty window, "Window error 1": its trace passes untouched), with both -- each under both
penalties.  No element and no trace is exempted.

The kernel is bounded on IDENTICAL float32 inputs: the reference is fed the library's own fwi_ops.condition output of obs, syn and d, and
its result, rounded to float32, goes through the library's own C^T.  Both stages are shipped and held by their own tests.  The bounds
follow from "double arithmetic, rounded once" (EPS = 2^-24, the relative rounding error of float32):
    misfit        |f - f_ref| <= 8 EPS f_ref                 (the bound of tests/test_gpu_w2_data.py for its sum)
    window sets   per sample |a - a_ref| <= 2 EPS |a_ref|     (one float32 rounding, and a factor of two for the operation order in double);
                  exactly 0 on dead traces and at sample 0
    filter sets   |a - a_ref| <= 16 EPS |a_ref| in rel-L2     (the outputs pass through the float32 transposed band-pass: the bound of
                  tests/test_gpu_w2_data.py under filter); exactly 0 on dead traces
The scale A is checked EXACTLY: with robust_delta = 1/2 (a power of two) and a synthetic gather far from the observed one every sample
where the taper is 1 sits on Huber's plateau, res = -+delta there, and |res| / robust_delta must be np.sort(|C obs|[1:])[k] bit for bit.
Symmetry of data_gn_obs: with fl(C x) = C x + e, |e| <= kappa EPS |C| |x| for the float32 window and band-pass (kappa ~ 4: nine
butterfly stages at 514 points), <u, G v> - <v, G u> is bounded by 4 kappa EPS |C|^2 |u| |v|: the bound is 32 EPS cmax^2 |u| |v|, cmax the
largest amplitude weight of the windows (1 without if_win).
Every comparison prints its deviation before it asserts; profiles/r29_robust_misfit.txt holds the figures measured on the MI355X.

On the parent commit every test fails: the keys are unknown there (and fwi_ops.data_gn has no obs)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cond_gn_ref as G
import data_entry_common as DC
import envelope_ref as E
import robust_ref as R
from data_entry_common import flat, traces, unflat

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
MISFIT_EPS, SAMPLE_EPS, L2_EPS, SYM_EPS = 8 * EPS, 2 * EPS, 16 * EPS, 32 * EPS
NSTEPS = (2, 3, 64, 65, 257, 1025)
LAYOUTS = {"one": (1,), "five": (5,), "ragged": (5, 3)}
FILTER = [25.0, 60.0, 260.0, 400.0]      # tests/test_gpu_envelope_data.py's: the lower ramp cuts into the traces' 25 ... 175 Hz
KEYSETS = {"alone": {}, "filter": {"filter": FILTER}, "window": {"if_win": True}, "both": {"filter": FILTER, "if_win": True}}
DELTA = 0.5                              # a power of two: delta A is a float32 whenever A is; about half the samples of the traces lie outside


def problem(tmp, nt, layout, keys, name, kind="huber", delta=DELTA, q=None, plain=False):
    nrec = LAYOUTS[layout] if isinstance(layout, str) else layout
    more = {} if plain else {R.KEY: kind, R.DELTA_KEY: delta}
    if q is not None:
        more[R.Q_KEY] = q
    return DC.problem(tmp, nt, nrec, dict(KEYSETS[keys], **more), name, misfit_key=None)


def cond(hip_ops, pb, gathers, transpose=False):
    return unflat(hip_ops.condition(flat(gathers).cuda(), pb["Shot_ids"], pb["para_fname"], transpose=transpose), gathers)


def misfit(hip_ops, pb, obs, syn, ids=None):
    f, a = hip_ops.data_misfit(flat(obs).cuda(), flat(syn).cuda(), pb["Shot_ids"] if ids is None else ids, pb["para_fname"])
    return f, unflat(a, obs)


def gn_obs(hip_ops, pb, obs, syn, d):
    return unflat(hip_ops.data_gn(flat(syn).cuda(), flat(d).cuda(), pb["Shot_ids"], pb["para_fname"], obs=flat(obs).cuda()), d)


def compare(got, ref, dead, filtered, what):
    """-> (worst per-sample gap in units of |ref|, rel-L2, what misses the bound of the key set or the exact zeros: asserted empty by the
    caller once the figures are printed)"""
    worst, num, den, bad = 0.0, 0.0, 0.0, []
    for x, y, dd in zip(got, ref, dead):
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        gap = np.abs(x64 - y64)
        num, den = num + float((gap ** 2).sum()), den + float((y64 ** 2).sum())
        if not filtered:
            ok = gap <= SAMPLE_EPS * np.abs(y64)
            rel = np.where(y64 != 0, gap / np.where(y64 != 0, np.abs(y64), 1.0), np.where(gap == 0, 0.0, np.inf))
            worst = max(worst, float(rel.max()))
            if not ok.all():
                bad.append((what, "per sample", float(rel.max()) / EPS))
            if x[:, 0].any():
                bad.append((what, "sample 0"))
        if x[dd].any():
            bad.append((what, "a dead trace"))
    l2 = np.sqrt(num / den) if den > 0 else np.sqrt(num)
    if filtered and not l2 <= L2_EPS:
        bad.append((what, "rel-L2", l2 / EPS))
    return worst, l2, bad


# ---- against the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("nt", NSTEPS)
def test_misfit_adjoint_source_and_data_gn_obs_against_the_reference(hip_ops, tmp_path, nt, layout):
    for keys in KEYSETS:
        for kind in R.KINDS:
            hip_ops.release()
            pb = problem(tmp_path / keys / kind, nt, layout, keys, "rb", kind)
            obs, syn, d = traces(pb, 1), traces(pb, 2), traces(pb, 3)
            what = "nt %d %s %s %s" % (nt, layout, keys, kind)
            co, cs, cd = cond(hip_ops, pb, obs), cond(hip_ops, pb, syn), cond(hip_ops, pb, d)
            f_ref, psi, ws, As = R.conditioned_misfit(pb, co, cs)
            dead = [A == 0 for A in As]
            a_ref = cond(hip_ops, pb, [x.astype(np.float32) for x in psi], transpose=True)
            g_ref = cond(hip_ops, pb, [(w * x).astype(np.float32) for w, x in zip(ws, cd)], transpose=True)
            f, a = misfit(hip_ops, pb, obs, syn)
            g = gn_obs(hip_ops, pb, obs, syn, d)
            gap_f = abs(f - f_ref) / f_ref if f_ref > 0 else abs(f)
            filtered = "filter" in KEYSETS[keys]
            assert np.isfinite(f) and all(np.isfinite(x).all() for x in a + g), what
            wa, la, bad_a = compare(a, a_ref, dead, filtered, what + " adjoint source")
            wg, lg, bad_g = compare(g, g_ref, dead, filtered, what + " data_gn_obs")
            print("robust data %s: misfit %.8e (reference %.8e, gap %.2f EPS); adjoint source per-sample %.2f EPS, rel-L2 %.2f EPS; data_gn_obs per-sample "
                  "%.2f EPS, rel-L2 %.2f EPS; %d dead of %d traces" % (what, f, f_ref, gap_f / EPS, wa / EPS, la / EPS, wg / EPS, lg / EPS, sum(int(x.sum()) for x in dead), sum(x.size for x in dead)))
            assert not bad_a and not bad_g, bad_a + bad_g
            assert abs(f - f_ref) <= MISFIT_EPS * f_ref, (what, f, f_ref)
            if any((~x).any() for x in dead):      # (nSteps = 3 under if_win: the window leaves one live sample of two, k = 0 falls on the zero)
                assert f_ref > 0 and G.norm(a_ref) > 0 and G.norm(g_ref) > 0, what
            assert nt < 64 or any((~x).any() for x in dead), what
            if "if_win" in KEYSETS[keys] and max(LAYOUTS[layout]) > 1:
                assert all(x[1] for x in dead), what      # channel 1 has weight 0
    hip_ops.release()


# ---- the selection, exactly ---------------------------------------------------------------------------------------------------------------
def selection_gather(nt, rng):
    """six observed traces: band-limited; constant |o| with mixed signs (all ties); one nonzero sample; all zero; +-0 mixed with a few nonzero
    samples; four levels only (ties around every rank)"""
    o = np.zeros((6, nt), np.float32)
    o[0] = E.band_limited(rng, 1, nt)[0]
    o[1] = np.float32(0.75) * rng.choice([-1.0, 1.0], nt)
    o[2, nt // 2] = -0.625
    o[4] = rng.choice(np.asarray([0.0, -0.0, -0.0, 0.25, -0.5], np.float32), nt)
    o[4, 1 + (nt - 1) // 2] = 0.375      # (one nonzero sample at least, also at nt = 2)
    o[5] = rng.choice(np.asarray([0.125, -0.25, 0.5, -1.0], np.float32), nt)
    return o


@pytest.mark.parametrize("nt", NSTEPS)
def test_the_scale_is_the_exact_order_statistic(hip_ops, tmp_path, nt):
    """k = 0, k = n - 1 and ranks between; ties, a single live value, a dead trace, -0 = +0: |res| / robust_delta on the plateau equals
    np.sort(|C obs|[1:])[k] bit for bit, and a trace with A = 0 gives exact zeros"""
    rng = np.random.default_rng(23)
    obs = [selection_gather(nt, rng)]
    syn = [(obs[0] + np.float32(16.0)).astype(np.float32)]      # r = -16 taper: u <= -16 / (delta A), far out on the plateau (A <= 1.5)
    for q in (1e-9, 0.3, 0.5, 0.9, 0.999, 1.0):
        hip_ops.release()
        pb = problem(tmp_path / ("q%g" % q), nt, (6,), "alone", "sel", "huber", q=q)
        co = cond(hip_ops, pb, obs)[0]
        flat_one = cond(hip_ops, pb, [np.ones((6, nt), np.float32)])[0]
        A = np.asarray([R.scale(co[r], q) for r in range(6)], np.float32)
        f, a = misfit(hip_ops, pb, obs, syn)
        a = a[0]
        live = 0
        for r in range(6):
            on = np.flatnonzero(flat_one[r] == 1.0)      # where C and C^T multiply by exactly 1 (never sample 0)
            assert on.size >= 1 and on[0] >= 1
            got = np.abs(a[r, on]) / np.float32(DELTA)
            print("robust select nt %d q %g trace %d: k %d, A %.9g (bits %08x), read from the plateau %.9g" % (nt, q, r, R.rank(nt - 1, q), A[r], A[r].view(np.uint32), got[0]))
            if A[r] == 0:
                assert not a[r].any(), (nt, q, r)
                continue
            live += 1
            assert np.array_equal(got.view(np.uint32), np.full(on.size, A[r].view(np.uint32))), (nt, q, r, got[0], A[r])
            assert (a[r, on] < 0).all()
        assert live >= 2 and A[3] == 0 and (q < 1.0 or A[2] == np.float32(0.625)), (nt, q, A)
    hip_ops.release()


# ---- the L2 limit --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keys", ["filter", "window", "both"])
def test_a_large_delta_gives_the_plain_files_call(hip_ops, tmp_path, keys):
    """robust_delta = 1e6: every sample is inside (u^2 < 1e-9).  Huber's psi is float32(double(o) - double(s)), which is the float32
    difference o - s of l2_residual bit for bit (the double difference is exact, or o absorbs s in both); Cauchy's differs by the factor
    1 / (1 + u^2), a last place.  The sums differ in their order: the misfit bound.  (The key alone has no plain twin: the plain file has
    no end taper.)"""
    pb0 = problem(tmp_path / "plain", 257, "ragged", keys, "plain", plain=True)
    obs, syn, d = traces(pb0, 1), traces(pb0, 2), traces(pb0, 3)
    hip_ops.release()
    f0, a0 = misfit(hip_ops, pb0, obs, syn)
    g0 = unflat(hip_ops.data_gn(flat(syn).cuda(), flat(d).cuda(), pb0["Shot_ids"], pb0["para_fname"]), d)
    for kind in R.KINDS:
        hip_ops.release()
        pb = problem(tmp_path / kind, 257, "ragged", keys, "big", kind, delta=1e6)
        f, a = misfit(hip_ops, pb, obs, syn)
        g = gn_obs(hip_ops, pb, obs, syn, d)
        flips = sum(int((x != y).sum()) for x, y in zip(a, a0)), sum(int((x != y).sum()) for x, y in zip(g, g0))
        print("robust data delta 1e6 %s %s: misfit %.8e, plain file %.8e (gap %.2f EPS); adjoint source differs at %d samples, data_gn_obs at %d; rel-L2 %.2e / %.2e"
              % (keys, kind, f, f0, abs(f - f0) / f0 / EPS, flips[0], flips[1], DC.rel(a, a0), DC.rel(g, g0)))
        assert f0 > 0 and abs(f - f0) <= MISFIT_EPS * f0
        if kind == "huber":
            assert flips == (0, 0)
        else:
            assert DC.rel(a, a0) <= L2_EPS and DC.rel(g, g0) <= L2_EPS
    hip_ops.release()


# ---- symmetry ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("keys", list(KEYSETS))
def test_data_gn_obs_is_symmetric_and_non_negative(hip_ops, tmp_path, keys, kind):
    hip_ops.release()
    pb = problem(tmp_path, 257, "ragged", keys, "sym", kind)
    obs, syn, u, v = (traces(pb, k) for k in (1, 2, 3, 4))
    gu, gv = gn_obs(hip_ops, pb, obs, syn, u), gn_obs(hip_ops, pb, obs, syn, v)
    uu, vv, uv, vu = G.dot(u, gu), G.dot(v, gv), G.dot(u, gv), G.dot(v, gu)
    cmax = 1.0
    if "if_win" in KEYSETS[keys]:
        cmax = max(max(sh["weights"]) * sh["src_weight"] for sh in (pb["survey"]["shot%d" % s] for s in G.shots_of(pb)))
    scale = cmax ** 2 * G.norm(u) * G.norm(v)
    print("robust data symmetry %s %s: <u, G u> %.8e, <v, G v> %.8e, <u, G v> %.8e, <v, G u> %.8e, gap %.2f EPS of cmax^2 |u| |v| (cmax %.3f)"
          % (keys, kind, uu, vv, uv, vu, abs(uv - vu) / scale / EPS, cmax))
    assert uu > 0 and vv > 0 and abs(uv - vu) <= SYM_EPS * scale
    hip_ops.release()


# ---- the new entry under the files of before ---------------------------------------------------------------------------------------------
def raw_gn_obs(pb, obs, syn, d):
    """sepfwi_data_gn_obs itself, obs a tensor or None (NULL)"""
    from sepfwi import _native
    out = torch.empty_like(d)
    ids = np.ascontiguousarray(np.asarray(pb["Shot_ids"], np.int32)).reshape(-1)
    code = _native.lib().sepfwi_data_gn_obs(_native.ptr(out), _native.ptr(obs) if obs is not None else None, _native.ptr(syn), _native.ptr(d), 0, int(ids.size),
                                            C.c_void_p(ids.ctypes.data), str(pb["para_fname"]).encode(), _native.stream_arg(d.device))
    torch.cuda.synchronize()
    return code, out


@pytest.mark.parametrize("file", ["plain", "window", "both", "envelope"])
def test_data_gn_obs_without_obs_is_data_gn_under_the_files_of_before(hip_ops, tmp_path, file):
    hip_ops.release()
    if file == "envelope":
        pb = DC.problem(tmp_path, 257, (5, 3), KEYSETS["both"], "env")
    else:
        pb = DC.problem(tmp_path, 257, (5, 3), {} if file == "plain" else KEYSETS[file], "l2", misfit_key=None)
    obs, syn, d = (flat(traces(pb, k)).cuda() for k in (1, 2, 3))
    ref = hip_ops.data_gn(syn, d, pb["Shot_ids"], pb["para_fname"])
    code, out = raw_gn_obs(pb, None, syn, d)
    code2, out2 = raw_gn_obs(pb, obs, syn, d)
    assert code == 0 and code2 == 0 and ref.abs().max() > 0 and torch.equal(out, ref) and torch.equal(out2, ref)
    assert torch.equal(hip_ops.data_gn(syn, d, pb["Shot_ids"], pb["para_fname"], obs=obs), ref)
    hip_ops.release()


def test_refusals(hip_ops, tmp_path):
    """the old entry under the key names the new one; the new one needs obs under the key; both as SEPFWI_EINVAL, nothing written"""
    from sepfwi import _native
    hip_ops.release()
    pb = problem(tmp_path, 64, "five", "both", "ref")
    obs, syn, d = (flat(traces(pb, k)).cuda() for k in (1, 2, 3))
    with pytest.raises(_native.SepFwiError) as e:
        hip_ops.data_gn(syn, d, pb["Shot_ids"], pb["para_fname"])
    assert e.value.code == -1 and "sepfwi_data_gn_obs" in str(e.value) and "robust_misfit" in str(e.value)
    code, out = raw_gn_obs(pb, None, syn, d)
    assert code == -1 and "obs must not be NULL" in _native.lib().sepfwi_last_error().decode()
    code, out = raw_gn_obs(pb, obs, syn, d)
    assert code == 0 and out.abs().max() > 0
    hip_ops.release()


# ---- pointers, repeatability ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_host_and_device_pointers_and_a_second_call_give_the_same_bits(hip_ops, tmp_path, kind):
    hip_ops.release()
    pb = problem(tmp_path, 1025, "ragged", "both", "bits", kind)
    obs, syn, d = (flat(traces(pb, k)) for k in (1, 2, 3))
    keep = [t.clone() for t in (obs, syn, d)]
    ids, fn = pb["Shot_ids"], pb["para_fname"]
    fd, ad = hip_ops.data_misfit(obs.cuda(), syn.cuda(), ids, fn)
    fh, ah = hip_ops.data_misfit(obs, syn, ids, fn)
    f2, a2 = hip_ops.data_misfit(obs.cuda(), syn.cuda(), ids, fn)
    gd = hip_ops.data_gn(syn.cuda(), d.cuda(), ids, fn, obs=obs.cuda())
    gh = hip_ops.data_gn(syn, d, ids, fn, obs=obs)
    g2 = hip_ops.data_gn(syn.cuda(), d.cuda(), ids, fn, obs=obs.cuda())
    assert ad.is_cuda and not ah.is_cuda and ad.abs().max() > 0 and gd.is_cuda and not gh.is_cuda and gd.abs().max() > 0
    assert fd == fh == f2 and torch.equal(ad.cpu(), ah) and torch.equal(ad, a2) and torch.equal(gd.cpu(), gh) and torch.equal(gd, g2)
    assert all(torch.equal(a, b) for a, b in zip(keep, (obs, syn, d))), "an input was changed"
    hip_ops.release()
