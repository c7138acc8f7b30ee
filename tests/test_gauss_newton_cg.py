"""obj_wrapper.gauss_newton_cg -- the matrix-free preconditioned conjugate gradients of the Gauss-Newton step -- on the CPU, with a small
dense H split over three "parameter" tensors, against numpy in float64: numpy.linalg.solve for the converged step, and a plain textbook
PCG (ref_pcg below, float64) for everything that depends on the iteration (history, the non-positive-curvature exit, the cap)."""
import numpy as np
import pytest
import torch

from sepfwi.obj_wrapper import gauss_newton_cg

SHAPES = ((2, 3), (4,), (3, 2))     # 16 unknowns over three tensors
N = 16
EPS32 = 2.0 ** -24


def split(x, dtype=torch.float32):
    out, off = [], 0
    for s in SHAPES:
        n = int(np.prod(s))
        out.append(torch.tensor(np.asarray(x[off:off + n]).reshape(s), dtype=dtype))
        off += n
    return out


def join(ts):
    return np.concatenate([t.detach().double().numpy().ravel() for t in ts])


def spd(rng, eigs):
    q, _ = np.linalg.qr(rng.standard_normal((N, N)))
    return (q * np.asarray(eigs)) @ q.T


class Op:
    """hessvec of a dense H in float32, counting its calls"""

    def __init__(self, H):
        self.H, self.calls = torch.tensor(H, dtype=torch.float32), 0

    def __call__(self, v):
        assert isinstance(v, tuple) and len(v) == 3
        self.calls += 1
        x = torch.cat([t.reshape(-1) for t in v])
        return tuple(split((self.H @ x).numpy()))


def ref_pcg(H, g, damping=0.0, D=None, minv=None, maxiter=10, rtol=1e-2):
    """Textbook PCG on (H + damping D) p = -g in float64 -> (p, history, products); stops at non-positive curvature with the step found
    so far (the preconditioned steepest-descent direction if it is the first iteration)."""
    A = H + damping * np.diag(np.ones(N) if D is None else D)
    minv = np.ones(N) if minv is None else minv
    p, r = np.zeros(N), -g.copy()
    z = minv * r
    d, rz = z.copy(), float(r @ z)
    rz0, hist, calls = rz, [1.0], 0
    if not rz0 > 0:
        return p, hist, calls
    for it in range(maxiter):
        Ad = A @ d
        calls += 1
        curv = float(d @ Ad)
        if not curv > 0:
            if it == 0:
                p = d.copy()
            break
        alpha = rz / curv
        p, r = p + alpha * d, r - alpha * Ad
        z = minv * r
        rz_new = float(r @ z)
        hist.append(float(np.sqrt(max(rz_new, 0.0) / rz0)))
        if hist[-1] <= rtol:
            break
        d, rz = z + (rz_new / rz) * d, rz_new
    return p, hist, calls


@pytest.mark.parametrize("with_diag", [False, True])
def test_the_step_converges_to_the_damped_solve(with_diag):
    """-(H + lambda D)^-1 g from numpy.linalg.solve in float64.  Margin: a float32 product with a 16 x 16 matrix carries a relative
    error of up to 16 eps (eps = 2^-24); the accuracy conjugate gradients can attain is that times the condition number of the system
    (here about 1e2), and 4 x for the float32 updates of step and residual on top: 64 eps cond."""
    rng = np.random.default_rng(3)
    H = spd(rng, np.logspace(0.0, 2.0, N))
    g = rng.standard_normal(N)
    D = rng.uniform(0.5, 2.0, N) if with_diag else None
    lam = 0.3
    A = H + lam * np.diag(np.ones(N) if D is None else D)
    want = np.linalg.solve(A, -g)
    op = Op(H)
    p, hist = gauss_newton_cg(op, split(g), damping=lam, diag=None if D is None else split(D), maxiter=4 * N, rtol=1e-7)
    err = np.linalg.norm(join(p) - want) / np.linalg.norm(want)
    bound = 64.0 * EPS32 * np.linalg.cond(A)
    print("gauss_newton_cg diag %r: %d products, relative residual %.1e, step error %.2e (bound %.2e)" % (with_diag, op.calls, hist[-1], err, bound))
    assert [tuple(t.shape) for t in p] == list(SHAPES) and all(t.dtype == torch.float32 for t in p)
    assert err <= bound, (err, bound)
    assert hist[0] == 1.0 and len(hist) == op.calls + 1


def test_history_starts_at_one_and_does_not_increase_for_spd_h():
    """The history is that of the float64 textbook iteration on the same system (to float32 round-off times the condition number, as
    above), entry 0 is exactly 1 and, for this well-conditioned H (condition number 8), no entry exceeds the one before it -- in the
    reference iteration as well, so this is a property of the problem that the code must reproduce."""
    rng = np.random.default_rng(5)
    H = spd(rng, np.linspace(1.0, 8.0, N))
    g = rng.standard_normal(N)
    D = rng.uniform(0.5, 2.0, N)
    seen = []
    p, hist = gauss_newton_cg(Op(H), split(g), damping=0.1, diag=split(D), maxiter=8, rtol=0.0, callback=lambda it, r: seen.append((it, r)))
    _, want, _ = ref_pcg(H, g, damping=0.1, D=D, minv=1.0 / D, maxiter=8, rtol=0.0)
    assert hist[0] == 1.0 and len(hist) == 9 == len(want)
    assert all(b <= a for a, b in zip(want, want[1:]))
    assert all(b <= a for a, b in zip(hist, hist[1:])), hist
    assert seen == list(enumerate(hist[1:], start=1))
    tol = 64.0 * EPS32 * np.linalg.cond(H + 0.1 * np.diag(D))
    assert np.abs(np.asarray(hist) - np.asarray(want)).max() <= tol, (hist, want)


def test_zero_entries_of_the_preconditioner_are_floored():
    """diag with zeros (outside the illuminated region): M is floored at 1e-12 of the tensor's maximum, a tensor that is zero
    throughout at 1 -- no inf, no nan, and the first step is the float64 one with that M."""
    rng = np.random.default_rng(7)
    H = spd(rng, np.linspace(1.0, 4.0, N))
    g = rng.standard_normal(N)
    D = rng.uniform(0.5, 2.0, N)
    D[[0, 4]] = 0.0             # a zero in the first tensor (6 entries)
    D[6:10] = 0.0               # the second tensor (4 entries) entirely
    floor = np.concatenate([np.full(6, 1e-12 * D[:6].max()), np.ones(4), np.full(6, 1e-12 * D[10:].max())])
    minv = 1.0 / np.maximum(D, floor)
    for maxiter in (1, 6):
        p, hist = gauss_newton_cg(Op(H), split(g), diag=split(D), maxiter=maxiter, rtol=0.0)
        assert all(torch.isfinite(t).all() for t in p) and np.isfinite(hist).all(), (p, hist)
    p, hist = gauss_newton_cg(Op(H), split(g), diag=split(D), maxiter=1, rtol=0.0)
    want, want_hist, _ = ref_pcg(H, g, minv=minv, maxiter=1, rtol=0.0)
    # one step alpha d with d = -M^-1 g: float32 entries of d (eps each), a float32 product of 16 terms in alpha (16 eps), 4 x
    assert np.linalg.norm(join(p) - want) <= 64.0 * EPS32 * np.linalg.norm(want), (join(p), want)
    assert np.abs(want).max() > 1e6 * np.abs(want).min() and abs(hist[1] - want_hist[1]) <= 1e-4 * want_hist[1]
    # negative entries count as zero
    Dn = D.copy()
    Dn[0] = -3.0
    pn, _ = gauss_newton_cg(Op(H), split(g), diag=split(Dn), maxiter=1, rtol=0.0)
    assert all(torch.equal(a, b) for a, b in zip(p, pn))


def test_non_positive_curvature_on_the_first_iteration_returns_scaled_steepest_descent():
    rng = np.random.default_rng(9)
    g = rng.standard_normal(N)
    D = rng.uniform(0.5, 2.0, N)
    op = Op(-np.eye(N))
    p, hist = gauss_newton_cg(op, split(g), diag=split(D), maxiter=5)
    assert op.calls == 1 and hist == [1.0]
    want = [-(a / b) for a, b in zip(split(g), split(D))]
    for a, b in zip(p, want):
        assert torch.allclose(a, b, rtol=4 * EPS32, atol=0.0), (a, b)
    op = Op(-np.eye(N))
    p, hist = gauss_newton_cg(op, split(g), maxiter=5)          # no preconditioner: -g itself
    assert op.calls == 1 and hist == [1.0] and all(torch.equal(a, -b) for a, b in zip(p, split(g)))


def test_non_positive_curvature_on_a_later_iteration_returns_the_step_found_so_far():
    """H with one negative eigenvalue along a direction the gradient barely sees: the first search directions have positive curvature,
    a later one does not.  The float64 iteration says after how many products that happens and what the step is by then."""
    rng = np.random.default_rng(11)
    eigs = np.linspace(1.0, 3.0, N)
    eigs[-1] = -2.0
    q, _ = np.linalg.qr(rng.standard_normal((N, N)))
    H = (q * eigs) @ q.T
    g = q @ np.concatenate([rng.uniform(0.5, 1.0, N - 1), [1e-2]])
    want, want_hist, want_calls = ref_pcg(H, g, maxiter=12, rtol=0.0)
    assert 1 < want_calls < 12 and len(want_hist) == want_calls       # the last product met the negative curvature and added no entry
    op = Op(H)
    p, hist = gauss_newton_cg(op, split(g), maxiter=12, rtol=0.0)
    assert op.calls == want_calls and len(hist) == want_calls, (op.calls, want_calls, hist)
    assert np.linalg.norm(want) > 0
    # the step is that of the iterations before the exit, all of positive curvature: the margin of the converged solve above with the
    # condition number 3 of the positive part, 64 eps x 3 = 1.1e-5 (measured: 1.6e-7)
    err = np.linalg.norm(join(p) - want) / np.linalg.norm(want)
    print("gauss_newton_cg, exit at product %d: step error %.2e" % (op.calls, err))
    assert err <= 64.0 * EPS32 * 3.0, (join(p), want)


def test_maxiter_caps_the_number_of_products():
    rng = np.random.default_rng(13)
    H = spd(rng, np.logspace(0.0, 2.0, N))
    for cap in (1, 3):
        op = Op(H)
        p, hist = gauss_newton_cg(op, split(rng.standard_normal(N)), maxiter=cap, rtol=0.0)
        assert op.calls == cap and len(hist) == cap + 1
    op = Op(H)
    p, hist = gauss_newton_cg(op, split(rng.standard_normal(N)), maxiter=0)
    assert op.calls == 0 and hist == [1.0] and all(not t.any() for t in p)


def test_a_zero_gradient_returns_zeros():
    op = Op(np.eye(N))
    p, hist = gauss_newton_cg(op, split(np.zeros(N)), diag=split(np.ones(N)), damping=0.5)
    assert op.calls == 0 and hist == [1.0]
    assert [tuple(t.shape) for t in p] == list(SHAPES) and all(not t.any() for t in p)
