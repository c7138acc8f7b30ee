"""What licenses tests/w2_ref.py as the yardstick of the W2 misfit (no GPU): its hand-written gradient against torch float64 autograd of
the definition and against central differences, the properties the misfit is chosen for, and how far the deliberate errors that a kernel
could make move the result on the inputs of tests/test_gpu_w2_data.py.  Every figure is printed before it is asserted.

Bounds.  The definition is evaluated in float64 (eps 1.1e-16); 1 / g and the suffix sums amplify a relative input error by up to 1e2
(measured below), and a sum over n <= 600 samples adds a factor sqrt(n): 1e-12 of the largest entry bounds the distance between two
float64 evaluations in different orders (hand formula and autograd).  Central differences at step 1e-5 have a truncation error of the
step's square times the third derivative, 1e-10 of |a| |v| by measurement: the bound is 1e-8."""
import numpy as np
import pytest
import torch

import envelope_ref as E
import w2_ref as W

DT = 1.0e-3
SIZES = (2, 3, 5, 64, 65, 600)


def pair(n, seed=0):
    x = E.band_limited(np.random.default_rng(seed), 2, n)
    return x[0], x[1]


def torch_W(o, s, dt, beta):
    """the definition, term by term, in torch float64: -> (W, dW/ds by autograd)"""
    o = torch.tensor(np.asarray(o, np.float64))
    s = torch.tensor(np.asarray(s, np.float64), requires_grad=True)
    n, dt = o.shape[0], float(np.float32(dt))
    A = o.abs().max()
    q = lambda z: torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs()))
    qs, qo = q(beta * s[1:] / A), q(beta * o[1:] / A)
    ps, po = torch.cumsum(qs, 0), torch.cumsum(qo, 0)
    f, g = qs / ps[-1], qo / po[-1]
    F, Gc = ps / ps[-1], torch.cat([torch.zeros(1, dtype=torch.float64), po / po[-1]])
    j = torch.clamp(torch.searchsorted(Gc[1:].detach().contiguous(), F.detach().contiguous(), right=False) + 1, max=n - 1)
    t = torch.arange(1, n, dtype=torch.float64) * dt
    T = (j - 1).double() * dt + dt * (F - Gc[j - 1]) / g[j - 1]
    Wv = (f * (t - T) ** 2).sum()
    Wv.backward()
    return float(Wv.detach()), s.grad.numpy()


@pytest.mark.parametrize("beta", [3.0, 8.0])
@pytest.mark.parametrize("n", SIZES)
def test_hand_gradient_equals_autograd(n, beta):
    o, s = pair(n)
    p = W.trace_parts(o, s, DT, beta)
    Wt, gt = torch_W(o, s, DT, beta)
    top = max(float(np.abs(gt).max()), 1e-300)
    gap = float(np.abs(p["dWds"] - gt).max()) / top
    print("w2 reference n %d beta %g: W %.10e (autograd's %.10e), hand gradient against autograd %.2e of the largest entry" % (n, beta, p["W"], Wt, gap))
    assert abs(p["W"] - Wt) <= 1e-12 * max(Wt, 1e-300) and gap <= 1e-12 and p["dWds"][0] == 0.0


@pytest.mark.parametrize("n", [5, 65, 600])
def test_hand_gradient_meets_central_differences(n):
    o, s = pair(n)
    v = np.random.default_rng(3).standard_normal(n)
    v[0] = 0.0
    eps = 1e-5
    a = -0.5 * W.trace_parts(o, s, DT)["dWds"]
    fd = (0.5 * W.trace_parts(o, s.astype(np.float64) + eps * v, DT)["W"] - 0.5 * W.trace_parts(o, s.astype(np.float64) - eps * v, DT)["W"]) / (2 * eps)
    gap = abs(fd + float(a @ v)) / (np.linalg.norm(a) * np.linalg.norm(v))
    print("w2 reference n %d: central differences against -<a, v>: %.2e of |a| |v|" % (n, gap))
    assert gap <= 1e-8


def test_non_negative_and_zero_where_the_data_fit():
    o, s = pair(600)
    ind = W.trace_parts(o, s, DT)
    fit = W.trace_parts(o, o, DT)
    ratio = float(np.linalg.norm(fit["dWds"]) / np.linalg.norm(ind["dWds"]))
    print("w2 reference obs = syn: W %.2e (independent pair %.2e), |a| %.2e of the independent pair's" % (fit["W"], ind["W"], ratio))
    assert ind["W"] > 0 and 0 <= fit["W"] <= 1e-20 * ind["W"] and ratio <= 1e-10
    for seed in range(5):
        o, s = pair(257, seed)
        assert W.trace_parts(o, s, DT)["W"] >= 0


def test_a_common_power_of_two_changes_no_bit():
    o, s = pair(600)
    k = np.float32(2.0 ** -10)
    p, q = W.trace_parts(o, s, DT), W.trace_parts(o * k, s * k, DT)
    assert p["W"] == q["W"] and np.array_equal(p["dWds"] * 2.0 ** 10, q["dWds"])


def test_dead_and_one_sample_traces_give_nothing():
    o, s = pair(64)
    tot, a, Ws = W.gather(np.stack([np.zeros(64, np.float32), o]), np.stack([s, s]), DT)
    assert Ws[0] == 0 and not a[0].any() and Ws[1] > 0 and a[1].any()      # A == 0: dead
    o2, s2 = pair(2)
    p = W.trace_parts(o2, s2, DT)
    assert p["W"] == 0 and not p["dWds"].any()                             # nSteps = 2: one mass sample, both densities are that sample


def test_monotone_over_two_and_a_quarter_periods_where_l2_is_not():
    """a two-arrival 15 Hz Ricker trace shifted by 0 ... 150 ms: W strictly increasing at beta 3, 5 and 8, not at 2; L2 turns back"""
    shifts = [0.005 * k for k in range(31)]
    o = W.ricker_pair(600, DT, 15.0)
    curves = {}
    for beta in (2.0, 3.0, 5.0, 8.0):
        curves[beta] = [W.trace_parts(o.astype(np.float32), W.ricker_pair(600, DT, 15.0, shift=sh).astype(np.float32), DT, beta)["W"] for sh in shifts]
    l2 = [float(((o - W.ricker_pair(600, DT, 15.0, shift=sh)) ** 2).sum()) for sh in shifts]
    mono = {b: all(y > x for x, y in zip(c, c[1:])) for b, c in curves.items()}
    print("w2 reference shifts 0 ... 150 ms: monotone at beta %s; L2 monotone: %s" % (mono, all(y > x for x, y in zip(l2, l2[1:]))))
    assert mono[3.0] and mono[5.0] and mono[8.0] and not mono[2.0]
    assert not all(y > x for x, y in zip(l2, l2[1:]))
    assert W.BETA == 3.0


def gpu_inputs(oracle, n=257, nrec=5):
    """the traces of tests/test_gpu_w2_data.py (data_entry_common.traces: seeds 1 and 2) under the end taper"""
    o = oracle.cond_window(E.band_limited(np.random.default_rng(1), nrec, n), DT, None)
    s = oracle.cond_window(E.band_limited(np.random.default_rng(2), nrec, n), DT, None)
    return o, s


def test_inputs_discriminate(oracle):
    """on the GPU tests' inputs each of these errors moves the adjoint source by far more than the 16 x 2^-24 = 9.5e-7 those tests allow"""
    o, s = gpu_inputs(oracle)
    _, a, _ = W.gather(o, s, DT)
    na = np.linalg.norm(a)
    wrong = {"the L2 adjoint source": E.Z(o.astype(np.float64) - s), "psi without its suffix sum": np.zeros(a.shape),
             "no projection": np.zeros(a.shape), "A from syn": np.zeros(a.shape)}
    for r in range(o.shape[0]):
        p = W.trace_parts(o[r], s[r], DT)
        sig = np.zeros(o.shape[1])
        sig[1:] = W.sigmoid(W.BETA * s[r, 1:].astype(np.float64) / p["A"]) * (W.BETA / p["A"])
        psi0 = p["d"]
        wrong["psi without its suffix sum"][r, 1:] = -0.5 * sig[1:] * (psi0 - (p["f"] * psi0).sum()) / p["Ss"]
        wrong["no projection"][r, 1:] = -0.5 * sig[1:] * p["psi"] / p["Ss"]
        wrong["A from syn"][r] = -0.5 * W.trace_parts(o[r], s[r], DT, scale_from=s[r])["dWds"]
    for name, w in wrong.items():
        gap = np.linalg.norm(w - a) / na
        cos = float((w * a).sum() / (np.linalg.norm(w) * na))
        print("w2 reference, %s instead of a: rel-L2 %.3f, cosine %.3f" % (name, gap, cos))
        assert gap > 1e-2, name      # four orders above the GPU tests' bound


def test_amplification_of_an_input_perturbation(oracle):
    """how far a relative perturbation of obs and syn moves a and W: linear growth (1 / g and the suffix sums, no index flips)"""
    o, s = gpu_inputs(oracle, 600)
    tot, a, _ = W.gather(o, s, DT)
    rng = np.random.default_rng(9)
    out = {}
    for eta in (1e-7, 3e-5):
        po = o.astype(np.float64) * (1.0 + eta * rng.standard_normal(o.shape))
        ps = s.astype(np.float64) * (1.0 + eta * rng.standard_normal(s.shape))
        t2, a2, _ = W.gather(po, ps, DT)
        out[eta] = (np.linalg.norm(a2 - a) / np.linalg.norm(a), abs(t2 - tot) / tot)
        print("w2 reference, a relative input perturbation of %.0e moves a by %.2e rel-L2 and W by %.2e" % (eta, *out[eta]))
    assert out[1e-7][0] < 1e-4 and out[3e-5][0] < 5e-2                      # amplified, by at most 1e3
    assert 30 < out[3e-5][0] / out[1e-7][0] < 3000                         # ... and linearly (300 x the perturbation: 300 x the change, within 10 x)
