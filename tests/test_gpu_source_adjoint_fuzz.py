"""Seeded random small problems for the source block of the exact adjoint (-m gpu): sepfwi_adjoint_exact_src against J itself outside the
GPU, on the default seeds and draws of tests/test_gpu_exact_adjoint_fuzz.py (fuzz_draws.draw_problem / draw_born / draw_exact: channels
inside the absorbing strips, ragged channel counts, joint weights, gauge lengths, a water layer, padded widths below 64, nPad 0 ... 8 with
dz != dx, the draw's kernel options) with two seeded source perturbations ds1, ds2 per draw (stf_ref.draw_ds: white plus smooth, about
2 % of the wavelet so that J_s ds is of the size of J_m v, first and last samples non-zero).

Reference (stf_ref.source_oracle_side, no GPU; tests/test_stf_reference.py runs it on the default seeds and holds the number of draws
without a target at a quarter at most): J_m v, J_m d and w = W J_m d are fuzz_sides.exact_oracle_side's (tests/born_ref.py), J_s ds is the
oracle's own gathers with stf = ds (stf_ref.js_ref), all on both oracle builds; dot products in float64.  Tolerance, none new
(exact_adjoint_ref.held): |got - ref| <= 1e-3 scale + 3 |ref_nvfma - ref|.
    <ds1, g_stf>            = <J_s ds1, w>, all shots and the one live shot alone on its own scale     (identity 2)
    <v, g_m> + <ds1, g_stf> = <J_m v + J_s ds1, w>; g_m has sepfwi_adjoint_exact's bits
    u^T H u                 = |W^1/2 J u|^2 for u = [v; ds1] and [0; ds1]                                 (identity 3)
    <u1, H u2>              = <H u1, u2> = <W J u1, J u2> for u1 = [v; ds1], u2 = [d; ds2]
    [v; 0]                  the model blocks are the existing product's bits
A draw without a live record or without a target is reported (xfail) for the reasons fuzz_common.settled already allows, never passed."""
import numpy as np
import pytest

import exact_adjoint_ref as X
import fuzz_common as C
import problems as P
import stf_ref as S
from born_ref import COMPS
from exact_adjoint_ref import held
from fuzz_sides import describe_exact

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", list(C.DEFAULT_SEEDS))
def test_random_problem_source_block(tmp_path, oracle, oracle_nvfma, hip_ops, seed):
    o, scale = C.settled(S.source_oracle_side, tmp_path, oracle, oracle_nvfma, seed, "the record is not live (exact_oracle_side)")
    d, b, ref, src = o["d"], o["b"], o["ref"], o["src"]
    pb = d["pb"]
    fn, ids = pb["para_fname"], pb["Shot_ids"].numpy()
    tag = "source fuzz seed %d (%s)" % (seed, describe_exact(o, scale))
    if not o["target"]:
        pytest.xfail("seed %d: no target -- the two oracle builds differ by %r of the scales" % (seed, dict(o["yard"], **src["yard"])))
    cmp = src["cmp"]
    v, dm, ds1, ds2 = o["v"], o["dm"], src["ds1"], src["ds2"]
    loc1, loc2 = S.local_rows(ds1, ids), S.local_rows(ds2, ids)
    w = {c: np.concatenate([sh[c].reshape(-1) for sh in ref["w"]]) for c in COMPS if c in ref["w"][0]}
    hip_ops.release()
    with P.kernel_options(**b["opts"]):
        g, gs, _ = S.exact_src(pb, fn, w=w)
        g0, _, _ = S.exact_src(pb, fn, w=w, gstf=False, src_entry=False)
        h1, hs1, _ = S.exact_src(pb, fn, v=v, ds=ds1)
        h2, hs2, _ = S.exact_src(pb, fn, v=dm, ds=ds2)
        _, hs0, _ = S.exact_src(pb, fn, ds=ds1)
        hv, hvs, _ = S.exact_src(pb, fn, v=v)
        hv0, _, _ = S.exact_src(pb, fn, v=v, gstf=False, src_entry=False)
    hip_ops.release()
    for a in (gs, hs1, hs2, hs0, hvs):
        assert a.shape == (ids.size, pb["nSteps"]) and np.isfinite(a).all() and not np.any(a[:, -1]), tag
    # identity 2
    assert all(np.array_equal(x, y) for x, y in zip(g, g0)), (tag, "g_m must keep sepfwi_adjoint_exact's bits")
    one = o["one"]
    for key, got in (("<ds,gstf>", S.stf_dot(loc1, gs)), ("<ds,gstf> shot %d" % one, S.stf_dot(loc1, gs, [one])),
                     ("<[v;ds],JTw>", X.model_dot(v, g) + S.stf_dot(loc1, gs))):
        r, a, s = cmp[key]
        held(got, r, a, "%s %s" % (tag, key), scale=s)
    # identity 3
    assert all(np.array_equal(x, y) for x, y in zip(hv, hv0)), (tag, "[v; 0]: the model blocks must keep the existing product's bits")
    r, a, s = cmp["uHu [v;ds]"]
    held(X.model_dot(v, h1) + S.stf_dot(loc1, hs1), r, a, tag + " u^T H u, u = [v; ds]", scale=s)
    r, a, s = cmp["uHu [0;ds]"]
    held(S.stf_dot(loc1, hs0), r, a, tag + " u^T H u, u = [0; ds]", scale=s)
    c12 = X.model_dot(v, h2) + S.stf_dot(loc1, hs2)
    c21 = X.model_dot(dm, h1) + S.stf_dot(loc2, hs1)
    r, a, s = cmp["<u1,Hu2>"]
    held(c12, c21, c21 + (a - r), tag + " symmetry <u1, H u2> against <H u1, u2>", scale=s)
    held(c12, r, a, tag + " <u1, H u2> against <W J u1, J u2>", scale=s)
