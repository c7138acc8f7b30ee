"""What licenses tests/robust_ref.py as the yardstick of the robust misfits (no GPU): psi against torch float64 autograd of phi and
against central differences, the L2 limit, the properties of the IRLS operator, what the misfit is for (spikes), a dead trace, and how far
the deliberate errors that a kernel could make move the result on the inputs of tests/test_gpu_robust_data.py.  Every figure is printed
before it is asserted.

Bounds.  phi, psi and w are a handful of float64 operations per sample (eps 1.1e-16) and a sum over n <= 600 samples: 1e-13 of the largest
entry bounds the distance between two float64 evaluations in different orders (hand formula and autograd).  Central differences at step
h = 1e-6 |s| have a truncation error of h^2 phi''' ~ 1e-12 relative away from Huber's kink, and the kink (phi'' jumps at |u| = 1) costs one
sample's h phi'' where the step straddles it, 1e-6 of that sample: the bound is 1e-6 of |a| |v|.
L2 limit at robust_delta = 1e6: Huber is exactly the L2 branch when max |u| <= 1, up to the roundings of delta^2 (u^2 / 2) against r^2 / 2
(1e-14); Cauchy differs from L2 by the series' next term, u^2 / 2 in phi and u^2 in w, so its bound is max u^2 of the inputs (printed),
which is below 1e-9 for |r| < 30 A."""
import numpy as np
import pytest
import torch

import data_entry_common as DC
import envelope_ref as E
import robust_ref as R

DT = 1.0e-3
SIZES = (2, 3, 5, 64, 65, 600)
DELTAS = (0.05, 0.5, 4.0)      # most samples outside, a mix, most inside


def pair(n, seed=0, nrec=1):
    """-> (o, s), (nrec, n) float32 each"""
    x = E.band_limited(np.random.default_rng(seed), 2 * nrec, n)
    return x[:nrec], x[nrec:]


def torch_phi(o, s, kind, delta, q):
    """the definition in torch float64 -> (sum phi, d sum phi / ds by autograd); A from numpy's sort (a constant)"""
    A = R.scale(o, q)
    o = torch.tensor(np.asarray(o, np.float64))
    s = torch.tensor(np.asarray(s, np.float64), requires_grad=True)
    d = delta * A
    u = (o[1:] - s[1:]) / d
    if kind == "huber":
        phi = torch.where(u.abs() <= 1, d * d * 0.5 * u * u, d * d * (u.abs() - 0.5))
    else:
        phi = 0.5 * d * d * torch.log1p(u * u)
    tot = phi.sum()
    tot.backward()
    return float(tot.detach()), s.grad.numpy()


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_psi_equals_autograd_of_phi(n, kind):
    o, s = (x[0] for x in pair(n))
    for delta in DELTAS:
        for q in (0.9, 1.0, 1e-9):
            p = R.trace_parts(o, s, kind, delta, q)
            ft, gt = torch_phi(o, s, kind, delta, q)
            top = max(float(np.abs(gt).max()), 1e-300)
            gap = float(np.abs(-p["psi"] - gt).max()) / top
            print("robust reference %s n %d delta %g q %g: phi %.10e (autograd's %.10e), psi against autograd %.2e of the largest entry" % (kind, n, delta, q, p["phi"], ft, gap))
            assert abs(p["phi"] - ft) <= 1e-13 * max(ft, 1e-300) and gap <= 1e-13 and p["psi"][0] == 0.0 and p["w"][0] == 0.0
            assert ((p["w"][1:] > 0) & (p["w"][1:] <= 1)).all()


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("n", [5, 65, 600])
def test_psi_meets_central_differences(n, kind):
    o, s = (x[0] for x in pair(n))
    v = np.random.default_rng(3).standard_normal(n)
    for delta in DELTAS:
        a = R.trace_parts(o, s, kind, delta)["psi"]
        h = 1e-6 * float(np.abs(s).max())
        f = lambda x: R.trace_parts(o, x, kind, delta)["phi"]
        fd = (f(s.astype(np.float64) + h * v) - f(s.astype(np.float64) - h * v)) / (2 * h)
        gap = abs(fd + float(a[1:] @ v[1:])) / (np.linalg.norm(a) * np.linalg.norm(v))
        print("robust reference %s n %d delta %g: central differences against -<psi, v>: %.2e of |psi| |v|" % (kind, n, delta, gap))
        assert gap <= 1e-6


def test_the_scale_is_the_order_statistic_without_interpolation():
    o = np.asarray([9.0, -3.0, 1.0, -0.0, 2.0, -5.0, 4.0], np.float32)      # live |o|: 3 1 0 2 5 4 -> sorted 0 1 2 3 4 5
    for q, want in ((1e-9, 0.0), (0.2, 1.0), (0.39, 1.0), (0.4, 2.0), (0.9, 4.0), (0.99, 4.0), (1.0, 5.0)):
        assert R.scale(o, q) == want, (q, R.scale(o, q))
    assert R.scale(np.asarray([7.0, -2.5], np.float32), 0.9) == 2.5 and R.scale(np.asarray([7.0], np.float32)) == 0.0
    assert R.scale(np.full(9, -1.5, np.float32), 0.3) == 1.5      # all ties


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_large_delta_is_the_l2_misfit(kind):
    o, s = pair(600, nrec=5)
    d = E.band_limited(np.random.default_rng(5), 5, 600)
    tot, psi, w, A = R.gather(o, s, kind, 1e6)
    r = E.Z(o.astype(np.float64) - s)
    l2 = 0.5 * float((r * r).sum())
    umax2 = float((np.abs(r) / (1e6 * A[:, None])).max()) ** 2
    bound = 1e-14 if kind == "huber" else umax2
    gaps = (abs(tot - l2) / l2, np.abs(psi - r).max() / np.abs(r).max(), np.abs(w * d - E.Z(d.astype(np.float64))).max() / np.abs(d).max())
    print("robust reference %s at delta 1e6 against L2: misfit %.2e, adjoint source %.2e, data_gn %.2e (max u^2 %.2e, bound %.2e)" % ((kind,) + gaps + (umax2, bound)))
    assert umax2 < 1e-9 and all(g <= bound for g in gaps)


@pytest.mark.parametrize("kind", R.KINDS)
def test_the_irls_operator_is_symmetric_and_non_negative(oracle, tmp_path, kind):
    """in conditioned space G = Z diag(w) Z exactly; through the oracle's float32 C and C^T the two sides of each identity differ by the
    roundings of four float32 operators applied to 257-sample traces, a few 1e-7 each: the bound is 1e-5 of |u| |G v|"""
    pb = DC.problem(tmp_path, 257, (5, 3), {"if_win": True, R.KEY: kind, R.DELTA_KEY: 0.5}, "ref", misfit_key=None)
    obs, syn, u, v = (DC.traces(pb, k) for k in (1, 2, 3, 4))
    ids = range(len(obs))
    Gu, Gv = R.data_gn(oracle, pb, obs, syn, u), R.data_gn(oracle, pb, obs, syn, v)
    dot = lambda a, b: sum(float((np.asarray(x, np.float64) * np.asarray(y, np.float64)).sum()) for x, y in zip(a, b))
    nrm = lambda a: np.sqrt(dot(a, a))
    c = lambda gs: [R.C_of(oracle, pb, g, sid) for g, sid in zip(gs, ids)]
    co, cs, cu = c(obs), c(syn), c(u)
    _, _, ws, _ = R.conditioned_misfit(pb, co, cs)
    quad = sum(float((w * np.asarray(x, np.float64) ** 2).sum()) for w, x in zip(ws, cu))
    sym = abs(dot(u, Gv) - dot(v, Gu)) / (nrm(u) * nrm(Gv))
    pos = abs(dot(u, Gu) - quad) / quad
    print("robust reference %s IRLS operator: symmetry %.2e of |u| |Gv|, <u, Gu> = %.6e against sum w (Z C u)^2 = %.6e (gap %.2e)" % (kind, sym, dot(u, Gu), quad, pos))
    assert sym <= 1e-5 and pos <= 1e-5 and quad > 0 and all((w >= 0).all() and (w <= 1).all() and not w[:, 0].any() for w in ws)
    assert any((w[:, 1:] < 0.5).any() for w in ws) and any((w[:, 1:] > 0.9).any() for w in ws)      # both regimes are present


@pytest.mark.parametrize("kind", R.KINDS)
def test_spikes_move_the_robust_adjoint_source_by_delta_and_the_l2_one_by_themselves(kind):
    """m = 20 spikes of 100 x the trace's peak on samples above A (m < (1 - q) n = 60): A keeps its bits, psi changes at the m spiked samples
    alone and there by at most 2 delta (Huber: |psi| <= delta) or delta (Cauchy: |psi| <= delta / 2); the L2 adjoint source changes by the
    spikes themselves, 100 x the peak each"""
    n, m, delta = 600, 20, 0.5
    o, s = pair(n, nrec=5)
    spiked, where = R.add_spikes(o, m, np.random.default_rng(7))
    _, psi0, _, A0 = R.gather(o, s, kind, delta)
    _, psi1, _, A1 = R.gather(spiked, s, kind, delta)
    assert m < (1 - R.QUANTILE) * (n - 1) and np.array_equal(A0, A1) and (A0 > 0).all()
    cap = (2.0 if kind == "huber" else 1.0) * delta * A0
    for r in range(o.shape[0]):
        ch = np.abs(psi1[r] - psi0[r])
        l2 = np.abs((spiked[r].astype(np.float64) - s[r]) - (o[r].astype(np.float64) - s[r]))
        peak = float(np.abs(o[r]).max())
        print("robust reference %s, %d spikes, trace %d: psi moves at %d samples by at most %.3e (cap %.3e); the L2 source by %.3e, peak %.3e"
              % (kind, m, r, int((ch > 0).sum()), ch.max(), cap[r], l2.max(), peak))
        assert set(np.flatnonzero(ch)) <= set(where[r]) and ch.max() <= cap[r] * (1 + 1e-12)
        assert l2[where[r]].min() >= 98.0 * peak and np.linalg.norm(ch) <= np.sqrt(m) * cap[r] and np.linalg.norm(l2) >= 98.0 * peak * np.sqrt(m)


@pytest.mark.parametrize("kind", R.KINDS)
def test_a_dead_trace_among_live_ones(kind):
    o, s = pair(64, nrec=3)
    o = o.copy()
    o[1] = 0.0
    o[1, 0] = 3.0      # sample 0 is no live sample: the trace is dead all the same
    tot, psi, w, A = R.gather(o, s, kind, 0.5)
    live, _, _, _ = R.gather(o[[0, 2]], s[[0, 2]], kind, 0.5)
    assert A[1] == 0 and not psi[1].any() and not w[1].any() and A[0] > 0 and A[2] > 0 and psi[0].any() and psi[2].any() and tot == live
    # fewer than a tenth of the samples alive: the default quantile falls on a zero and the trace is dead; q = 1 revives it
    o[1, 5:9] = 1.0
    assert R.scale(o[1]) == 0.0 and R.scale(o[1], 1.0) == 1.0


def gpu_inputs(oracle, n=257, nrec=5, filt=None):
    """the traces of tests/test_gpu_robust_data.py (data_entry_common.traces: seeds 1 and 2, d: seed 3) under the end taper [and a filter]"""
    out = []
    for seed in (1, 2, 3):
        x = oracle.cond_window(E.band_limited(np.random.default_rng(seed), nrec, n), DT, None)
        out.append(oracle.cond_bandpass(x, DT, filt) if filt is not None else x)
    return out


@pytest.mark.parametrize("kind", R.KINDS)
def test_inputs_discriminate(oracle, kind):
    """on the GPU tests' inputs each of these errors moves the result by more than 1e-3 of its norm, four orders above the 2^-23 = 1.2e-7
    per sample that those tests allow.  Z shows under filter alone: the window's taper leaves sample 0 at zero, the band-pass after it does not."""
    delta = 0.5
    o, s, d = gpu_inputs(oracle)
    _, psi, w, _ = R.gather(o, s, kind, delta)
    gn = w * d
    wrong_psi, wrong_gn = np.zeros(psi.shape), np.zeros(psi.shape)
    for r in range(o.shape[0]):
        wrong_psi[r] = R.trace_parts(o[r], s[r], kind, delta, scale_from=s[r])["psi"]
    u = np.abs(o.astype(np.float64) - s) / (delta * R.gather(o, s, kind, delta)[3][:, None])
    true_hess = E.Z((u <= 1.0).astype(np.float64)) if kind == "huber" else E.Z((1 - u * u) / (1 + u * u) ** 2)
    wrong_gn = true_hess * d
    gaps = {"A from syn (adjoint source)": np.linalg.norm(wrong_psi - psi) / np.linalg.norm(psi),
            "w as the true Hessian (data_gn)": np.linalg.norm(wrong_gn - gn) / np.linalg.norm(gn)}
    of, sf, df = gpu_inputs(oracle, filt=[25.0, 60.0, 260.0, 400.0])
    _, psif, wf, Af = R.gather(of, sf, kind, delta)
    r0 = of[:, 0].astype(np.float64) - sf[:, 0]
    u0 = r0 / (delta * Af)
    w0 = np.minimum(1.0, 1.0 / np.maximum(np.abs(u0), 1e-300)) if kind == "huber" else 1.0 / (1.0 + u0 * u0)
    gaps["Z dropped (adjoint source, sample 0 under filter)"] = np.linalg.norm(r0 * w0) / np.linalg.norm(psif)
    gaps["Z dropped (data_gn, sample 0 under filter)"] = np.linalg.norm(w0 * df[:, 0]) / np.linalg.norm(wf * df)
    for name, gap in gaps.items():
        print("robust reference %s, %s: rel-L2 %.3e" % (kind, name, gap))
        assert gap > 1e-3, name
