"""What the GPU tests of the W2 misfit's kernel share (tests/test_gpu_w2_data.py, tests/test_gpu_w2_kernel_fuzz.py,
tests/test_gpu_w2_fuzz.py): the comparison of fwi_ops.data_misfit with tests/w2_ref.py on IDENTICAL float32 inputs, and its three bounds.

The map from the gathers to the adjoint source is ill-conditioned in its inputs and its derivative jumps where F_i crosses a node G_j, so
the kernel is never compared with an adjoint source derived from other gathers than its own: the reference is fed the library's own
fwi_ops.condition output of obs and syn, and its adjoint source, rounded to float32, goes through the library's own C^T.  The bounds
follow from "double arithmetic, rounded once" (EPS = 2^-24, the relative rounding error of float32) and hold for any input:
    misfit       |f - f_ref| <= 8 EPS f_ref                     (one rounding of the float32 result)
    window sets  per trace max |a - a_ref| <= 8 EPS max |a_ref|  (C^T pointwise: a one-place flip of the rounded source, carried through)
    filter sets  |a - a_ref| <= 16 EPS |a_ref|                   (C^T linear with norm <= 1, applied alike to both sides)"""
import numpy as np

import cond_gn_ref as G
import w2_ref as W
from data_entry_common import flat, unflat

EPS = 2.0 ** -24
MISFIT_EPS, TRACE_EPS, L2_EPS = 8 * EPS, 8 * EPS, 16 * EPS


def call(hip_ops, pb, obs, syn, ids=None):
    f, a = hip_ops.data_misfit(flat(obs).cuda(), flat(syn).cuda(), pb["Shot_ids"] if ids is None else ids, pb["para_fname"])
    return f, unflat(a, obs)


def deviations(f, a, f_ref, a_ref):
    """-> (misfit gap relative to f_ref, the largest per-trace max |a - a_ref| in units of max |a_ref|, rel-L2 of a, |a_ref|)"""
    gap_f = abs(f - f_ref) / f_ref if f_ref > 0 else abs(f)
    worst = 0.0
    for x, y in zip(a, a_ref):
        for r in range(x.shape[0]):
            top, d = float(np.abs(y[r]).max()), float(np.abs(x[r].astype(np.float64) - y[r]).max())
            worst = max(worst, d / top if top > 0 else (0.0 if d == 0 else np.inf))
    n_ref = G.norm(a_ref)
    gap_l2 = G.norm([x.astype(np.float64) - y for x, y in zip(a, a_ref)]) / n_ref if n_ref > 0 else G.norm(a)
    return gap_f, worst, gap_l2, n_ref


def on_identical_inputs(oracle, hip_ops, pb, obs, syn, what, ids=None):
    """the library against the reference on the library's own C obs, C syn; a file with a band-pass is held to the rel-L2 bound, one
    without to the per-trace bound; ids: a call on those shots alone (obs, syn then theirs).  -> (f, a, f_ref, a_ref) for further use"""
    fn = pb["para_fname"]
    ids = pb["Shot_ids"] if ids is None else ids
    sub = dict(pb, Shot_ids=ids)
    co = unflat(hip_ops.condition(flat(obs).cuda(), ids, fn), obs)
    cs = unflat(hip_ops.condition(flat(syn).cuda(), ids, fn), obs)
    f_ref, a64, _ = W.conditioned_misfit(oracle, sub, co, cs)
    a_ref = unflat(hip_ops.condition(flat([x.astype(np.float32) for x in a64]).cuda(), ids, fn, transpose=True), obs)
    f, a = call(hip_ops, pb, obs, syn, ids)
    gap_f, worst, gap_l2, n_ref = deviations(f, a, f_ref, a_ref)
    print("w2 data %s: misfit %.8e (reference %.8e, gap %.2f EPS), adj per-trace max gap %.2f EPS, rel-L2 %.2f EPS (|a| %.4e)"
          % (what, f, f_ref, gap_f / EPS, worst / EPS, gap_l2 / EPS, n_ref))
    assert np.isfinite(f) and all(np.isfinite(x).all() for x in a), what
    assert abs(f - f_ref) <= MISFIT_EPS * f_ref, (what, f, f_ref)
    if "filter" in pb["para"]:
        assert gap_l2 <= L2_EPS, (what, gap_l2 / EPS)
    else:
        assert worst <= TRACE_EPS, (what, worst / EPS)
    return f, a, f_ref, a_ref
