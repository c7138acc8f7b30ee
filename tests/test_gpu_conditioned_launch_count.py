"""sepfwi_stats.launches of a call under a live data-conditioning key is a COUNT (one per kernel, one per hipFFT exec), on the GPU (-m gpu).

A gradient call under a keyed file and one under the same file with "conditioning": "reference" (the keys are parsed and ignored, the plain
residual is one launch per shot) differ in nothing but the residual of every shot with channels, so the difference of their launches is
the chain's count minus 1 per such shot.  The count is written out below from the step lists at Conditioner::launches()
(csrc/conditioning.hpp); nothing is read from the library.

Problem: data_entry_common.problem -- 40 x 48, 10-cell layers, nSteps 65, two shots with 5 and 3 channels -- on the stream schedule.

Before the count the statistic was an estimate kept by hand (8 per shot, + 18 under the envelope key, whatever else was live), and every
case below failed -- the difference over the two shots was 14 where the count is 28 (L2 + both), 14 for 8 (L2 + window), 14 for 36
(cross + both), 50 for 64 (envelope + both), 50 for 44 (envelope + window), 14 for 60 (if_src_update + filter), and 176 for 174 in the
product (profiles/r25_conditioning_refactor.txt)."""
import pytest
import torch

import cond_gn_ref as G
import data_entry_common as DE
import envelope_ref as E
import problems as P

pytestmark = pytest.mark.gpu
NT, NREC = 65, (5, 3)
WINDOW, BANDPASS = 1, 5                      # bandpass: embed, R2C, the spectrum's multiplier, C2R, crop
MISFIT = {None: 1,                           # l2_residual
          "if_cross_misfit": 5,              # three norms, misfit, adjoint source
          E.KEY: 1 + 2 * 5 + 1 + 1 + 5 + 1}  # difference, two Hilbert transforms, residual, sum, a third transform, combination: 19
SOURCE_UPDATE, SOURCE_UPDATE_ADJ = 10, 6     # 2 embeds, 2 tapers, 2 R2C, coefficients, their product, C2R, crop / embed, R2C, conj, C2R, taper, crop
ENVELOPE_SCATTERED = 3 * 5 + 1 + 1           # three Hilbert transforms, the linearised residual, the combination: 17
CASES = {"l2_both": (None, "both", False), "l2_window": (None, "window", False), "cross_both": ("if_cross_misfit", "both", False),
         "envelope_both": (E.KEY, "both", False), "envelope_window": (E.KEY, "window", False), "src_update_filter": (None, "filter", True)}


def c_of(keys):
    return WINDOW + (BANDPASS if "filter" in E.KEYSETS[keys] else 0)


def chain(misfit_key, keys, src_update):
    """launches of one shot's residual under the file: 2 transposes, C, [source update], the misfit, [its transpose], C^T"""
    return 2 + c_of(keys) + (SOURCE_UPDATE if src_update else 0) + MISFIT[misfit_key] + (SOURCE_UPDATE_ADJ if src_update else 0) + c_of(keys)


def files(tmp, name, misfit_key, keys, src_update):
    """the keyed file and the same with "conditioning": "reference" """
    k = dict(E.KEYSETS[keys], **({"if_src_update": True} if src_update else {}))
    return (DE.problem(tmp / "keyed", NT, NREC, k, name, misfit_key), DE.problem(tmp / "ref", NT, NREC, dict(k, conditioning="reference"), name + "_ref", misfit_key))


def launches_of(hip_ops, pb, call):
    hip_ops.release()
    with P.kernel_options(batch=0):
        for sid, g in zip(G.shots_of(pb), DE.traces(pb, 5)):
            hip_ops.set_observed(pb["para_fname"], sid, torch.from_numpy(g))
        call(pb)
        n = hip_ops.stats(pb["para_fname"])["launches"]
    hip_ops.release()
    return n


def gradient(hip_ops):
    return lambda pb: hip_ops.backward(*[t.cuda() for t in pb["lame_init"]], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])


@pytest.mark.parametrize("case", list(CASES))
def test_gradient_call_counts_the_chain(hip_ops, tmp_path, case):
    misfit_key, keys, src_update = CASES[case]
    keyed, ref = files(tmp_path, case, misfit_key, keys, src_update)
    got = launches_of(hip_ops, keyed, gradient(hip_ops)) - launches_of(hip_ops, ref, gradient(hip_ops))
    want = sum(chain(misfit_key, keys, src_update) - 1 for n in NREC if n > 0)
    print("launch count %s: keyed - reference mode = %d, the chain's count - 1 over %d shots = %d" % (case, got, len(NREC), want))
    assert got == want


def test_envelope_product_counts_the_chain(hip_ops, tmp_path):
    """gauss_newton(exact=False) under envelope + both against the L2 + both product: per shot one more transposition and C of the background
    gather, and the linearised envelope (17) in the place of the one-kernel residual.  Session::born also records the background gather under
    the key, one sampler launch per time step and shot (record_background): that term is not the chain's and is written out
    separately."""
    env = DE.problem(tmp_path / "env", NT, NREC, E.KEYSETS["both"], "gn_env", E.KEY)
    l2 = DE.problem(tmp_path / "l2", NT, NREC, E.KEYSETS["both"], "gn_l2", None)

    def product(pb):
        m = [t.cuda() for t in pb["lame_init"]]
        v = [1e-3 * t for t in m]
        return hip_ops.gauss_newton(*m, *v, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"], exact=False)

    got = launches_of(hip_ops, env, product) - launches_of(hip_ops, l2, product)
    shots = sum(1 for n in NREC if n > 0)
    chain_more, recorded = shots * (1 + c_of("both") + ENVELOPE_SCATTERED - 1), shots * (NT - 1)
    print("launch count envelope product - L2 product = %d: the chain %d, the recorded background columns %d" % (got, chain_more, recorded))
    assert got == chain_more + recorded
