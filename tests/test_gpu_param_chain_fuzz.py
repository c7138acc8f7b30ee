"""The parameter chain's four kernels on random grids (-m gpu): k_param_jvp, k_param_diag + k_param_diag_rim and k_param_bwd +
k_param_bwd_rim of csrc/param_maps.hip through _MaskedTriple.tangent / diag / pullback, for every default seed x class of
tests/param_tangent_ref.py (draw_grid, fuzz_inputs).  The draws hold what the fixed grids of tests/test_gpu_param_tangent.py leave out: rim
cells with more replicas than the 64 lanes of their wave (up to three passes of `for (k = lane; k < cnt; k += 64)` and its k / w_, k % w_
split on a wide rectangle), one-row, one-column and two-row grids with padding, a strip of more than 64 cells under a bottom-row cell,
nPad without nPml, padded widths 63 ... 129, and masks that are fractional in the padding, so that the rim sums carry the blend with
the reference model (tests/test_param_chain_fuzz_reference.py holds the draws by a digest and counts all this on the CPU).

References and bounds, none new: the float64 torch.func.jvp of the modules' own expression for `tangent`; for `diag` E^T of its squares
(diag_ref64: no index arithmetic restated, equal to the dense Jacobian's on the tiny grids to 1e-12); for `pullback` the float64
autograd gradient of <chain(f), w>; each output array within tol_of (2e-6 algebraic kinds, 1e-6 rock physics) of its largest reference
entry; the transpose identity within the Hoelder sum of those.  A draw whose float32 torch path on the CPU does not leave room inside
the bound at any attempt (settled_inputs) is an xfail, never a pass; no default draw is one.  Every comparison prints its figure before
it asserts (profiles/r20_conditioned_and_param_chain_fuzz.txt holds those measured on the MI355X and what two wrong builds do to them)."""
import numpy as np
import pytest
import torch

import param_tangent_ref as T
from fuzz_common import seeds

pytestmark = pytest.mark.gpu


def _cuda(arrs):
    return [torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device="cuda") for a in arrs]


def _np(ts):
    return [t.detach().cpu().numpy() for t in ts]


@pytest.mark.parametrize("cls_name", T.CLASSES)
@pytest.mark.parametrize("seed", seeds("SEPFWI_PARAM_FUZZ"))
def test_random_grid_matches_float64_torch(hip_ops, seed, cls_name):
    o, attempt = T.settled_inputs(cls_name, seed)
    if o is None:
        pytest.xfail("seed %d %s: the float32 torch path leaves no room inside the bound at any of %d attempts" % (seed, cls_name, attempt))
    dims, mask_kind, f, mask, v, w, h = o
    nz, nx, nPml, nPad = dims
    tol = T.tol_of(cls_name)
    tag = "fuzz seed %d %s %s (%s mask, attempt %d)" % (seed, cls_name, "x".join(map(str, dims)), mask_kind, attempt)
    gpu = T.make_module(cls_name, dims, f, mask, device="cuda")
    m64 = T.make_module(cls_name, dims, f, mask, dtype=torch.float64)
    assert gpu._fusable()
    vc, wc, hc = _cuda(v), _cuda(w), _cuda(h)

    # the three operators against float64
    Pv = _np(gpu.tangent(*vc))
    assert all(a.shape == T.padded_shape(dims) for a in Pv)
    T.close(Pv, T.tangent64(m64, v), tol, tag + " tangent")
    d = _np(gpu.diag(*hc))
    assert all(a.shape == (nz, nx) for a in d)
    T.close(d, T.diag_ref64(m64, h), tol, tag + " diag")
    Ptw = _np(gpu.pullback(*wc))
    assert all(a.shape == (nz, nx) for a in Ptw)
    T.close(Ptw, T.pullback64(m64, w), tol, tag + " pullback")
    lhs, rhs = T.dot(Pv, w), T.dot(v, Ptw)
    bound = T.holder_bound(tol, Pv, w, Ptw, v)
    print("param tangent %s transpose identity: <P v, w> %.10e, <v, P^T w> %.10e, difference %.2e, bound %.2e" % (tag, lhs, rhs, abs(lhs - rhs), bound))
    assert abs(lhs) > 0 and abs(lhs - rhs) <= bound

    # asserted with ==
    zero = torch.zeros_like(vc[0])
    for keep in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)):
        a = _np(gpu.tangent(*[t if k else None for t, k in zip(vc, keep)]))
        b = _np(gpu.tangent(*[t if k else zero for t, k in zip(vc, keep)]))
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), keep
    assert not any(np.any(x) for x in a)                                     # v = 0
    assert all(np.isfinite(x).all() and not np.any(x[mask == 0]) for x in Pv)
    twice = _np(gpu.tangent(*[2.0 * t for t in vc]))
    assert all(np.array_equal(x, 2.0 * y) for x, y in zip(twice, Pv)) and any(np.any(y) for y in Pv)
    if cls_name == "FWI_Lame_Den":                                           # kind 1: P = diag(Mask) E
        from sepfwi import utils as ft
        assert all(np.array_equal(g, mask * ft.padding_numpy_array(a, nPml, nPad)) for g, a in zip(Pv, v))
    assert not any(np.any(x) for x in _np(gpu.diag(*[torch.zeros_like(t) for t in hc])))

    # a mask that is 0 on the whole padding: no rim term -- the same module without any padding, on the interior arrays
    inner = T.make_module(cls_name, dims, f, T.interior_mask(dims), device="cuda")
    bare = T.make_module(cls_name, (nz, nx, 0, 0), f, np.ones((nz, nx), np.float32), device="cuda")
    assert inner._fusable() and bare._fusable()
    crop = [a[nPml:nPml + nz, nPml:nPml + nx] for a in h]
    T.close(_np(inner.diag(*hc)), _np(bare.diag(*_cuda(crop))), tol, tag + " diag under the interior mask against the unpadded module")
