"""The W2 misfit's kernel alone on traces that are not band-limited noise, and across w2_beta (-m gpu): sepfwi_data_misfit through
fwi_ops.data_misfit under if_w2_misfit, no time loop, against tests/w2_ref.py on IDENTICAL float32 inputs (tests/w2_held.py: the
reference is fed the library's own fwi_ops.condition output, and its adjoint source goes through the library's own C^T).

Cases: every key set of tests/test_gpu_w2_data.py (the key alone, filter, if_win, both) x w2_beta 0.25, 1, 8, 16 (3 is that file's) x
nt 66, 257, 258, 1025 (the mass samples nt - 1 on both sides of a wave and of a tile of the block scans, and a fourth tile's carry).
Each case is ONE gather of seven channels, one trace kind per channel (w2_ref.trace_kinds), so that one launch mixes them:
    0  a band-limited pair (the kind of tests/test_gpu_w2_data.py, as the control)
    1  exact zeros up to 0.6 nt, then a Ricker arrival; the synthetic arrival at 0.3 nt: j(i) far from i, long flat densities
    2  synthetic = 1e3 x an independent band-limited trace: beta s / A in the thousands, exp underflows, sigmoid is exactly 0 on the
       negative side
    3  synthetic = 1e-3 x an independent trace
    4  synthetic all zeros beside a live observed trace: a uniform f
    5  observed = -|band-limited|, synthetic = +|band-limited|: one-signed; at beta 16 nodes of g near 1e-7, 1 / g_j near 1e7
    6  observed with one spike of 100 x its peak: A is the spike, both densities nearly flat, psi - P cancels
Under if_win data_entry_common.problem's rules stay: channel 1 has weight 0 (a dead trace: its row is exactly 0), the last channel the
empty window (its trace passes untouched).  The bounds are w2_held's, unchanged, for every kind: 8 EPS on the misfit, 8 EPS per trace
on the window sets, 16 EPS rel-L2 under filter ("double throughout, rounded once" holds for any input).  In addition every output is
finite, and host and device pointers and a second call give the same bits.

The condition on kinds 0 to 6: the reference decides every j(i) by a margin that its own summation order cannot move
(w2_ref.tie_margin >= 64 nt 2^-53 on every live trace); tests/test_w2_fuzz_reference.py asserts it on the CPU for both oracle builds' C.

The eighth kind, for the MISFIT only: the synthetic trace is the observed one delayed by three whole samples, with exact zeros at
both ends (on all seven channels of a second call).  Its F_i sit on the nodes G_(i+3) to within the order of summation, so j(i) is
decided by the last bit of two differently ordered sums -- the kernel's block scans and the reference's running sum.  The misfit is
continuous there (T_i is the same point of the inverse CDF read from either side of the node), the adjoint source is not (c_i changes
by the factor g_j / g_(j+1)): the misfit is held to 8 EPS, the output must be finite and repeat bit for bit, and the adjoint source is
not compared.

profiles/r31_w2_fuzz.txt holds the deviations measured on the MI355X."""
import numpy as np
import pytest
import torch

import cond_gn_ref as G
import w2_ref as W
from data_entry_common import flat, unflat
from test_gpu_w2_data import KEYSETS, problem
from w2_held import EPS, MISFIT_EPS, call, on_identical_inputs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("beta", W.FUZZ_BETAS)
@pytest.mark.parametrize("nt", W.FUZZ_NTS)
def test_trace_kinds_against_the_reference(oracle, hip_ops, tmp_path, nt, beta):
    kinds = W.trace_kinds(nt, W.kind_seed(nt, beta))
    for keys in KEYSETS:
        hip_ops.release()
        pb = problem(tmp_path / keys, nt, (7,), keys, "w2k", **{W.BETA_KEY: beta})
        ids, fn = pb["Shot_ids"], pb["para_fname"]
        obs, syn = [kinds["obs"]], [kinds["syn"]]
        what = "kinds nt %d beta %g %s" % (nt, beta, keys)
        f, a, f_ref, a_ref = on_identical_inputs(oracle, hip_ops, pb, obs, syn, what)
        live = [r for r in range(7) if np.abs(a_ref[0][r]).max() > 0]
        print("w2 kernel fuzz %s: live channels %r, per-channel max |a| %s" % (what, live, " ".join("%.2e" % np.abs(a[0][r]).max() for r in range(7))))
        assert f_ref > 0 and len(live) == (6 if "if_win" in pb["para"] else 7), (what, live)
        if "if_win" in pb["para"]:
            assert not a[0][1].any(), (what, "channel 1 has weight 0")
        fh, ah = hip_ops.data_misfit(flat(obs), flat(syn), ids, fn)
        f2, a2 = call(hip_ops, pb, obs, syn)
        assert not ah.is_cuda and f == fh == f2 and np.array_equal(ah.numpy(), flat(a).numpy()) and np.array_equal(a2[0], a[0]), what
        # the eighth kind: the misfit only (module docstring)
        so, ss = [kinds["shift_obs"]], [kinds["shift_syn"]]
        co = unflat(hip_ops.condition(flat(so).cuda(), ids, fn), so)
        cs = unflat(hip_ops.condition(flat(ss).cuda(), ids, fn), so)
        f8_ref, a8_64, _ = W.conditioned_misfit(oracle, pb, co, cs)
        a8_ref = unflat(hip_ops.condition(flat([x.astype(np.float32) for x in a8_64]).cuda(), ids, fn, transpose=True), so)
        f8, a8 = call(hip_ops, pb, so, ss)
        f8b, a8b = call(hip_ops, pb, so, ss)
        print("w2 kernel fuzz %s, a delay of %d whole samples: misfit %.8e (reference %.8e, gap %.2f EPS), |a| %.4e; for the record, not held: a against the reference's %.2e rel-L2"
              % (what, W.SHIFT, f8, f8_ref, abs(f8 - f8_ref) / f8_ref / EPS, G.norm(a8), G.norm([x.astype(np.float64) - y for x, y in zip(a8, a8_ref)]) / max(G.norm(a8_ref), 1e-300)))
        assert np.isfinite(f8) and np.isfinite(a8[0]).all() and f8_ref > 0, what
        assert abs(f8 - f8_ref) <= MISFIT_EPS * f8_ref, (what, f8, f8_ref)
        assert f8 == f8b and np.array_equal(a8[0], a8b[0]), what
    hip_ops.release()
