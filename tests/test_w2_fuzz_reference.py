"""What licenses tests/test_gpu_w2_kernel_fuzz.py (layer A) and tests/test_gpu_w2_fuzz.py (layer B) before any GPU run, on the CPU: what
draw_w2 draws and writes is held by a digest; every default draw has a live record, a build yardstick below the cap and an
amplification below 1e3 at some scale (so no default seed reaches the xfail branch on the GPU, as far as that can be known without
the library's own gathers: the plain oracle build's syn stands in their place for kappa); between them the draws hold what the fuzz is
for; every case of layer A decides every j(i) by a margin that no summation order can move; and the comparisons can fail -- five
weaker references each miss a bound of layer A by at least 5 x on a default case.

The generator's offset.  The mode of a seed belongs to draw_conditioned (filter: seeds 1, 2, 15; narrow: 3, 5, 11; window: 7, 9, 14;
both: the other seven) and its geometry, channels and option set to draw_problem and draw_born; draw_w2's own generator decides w2_beta,
which draws lose their conditioning keys, and on which draws one observed channel is silenced.  Sweeps of every (alone, w2_beta) pair
on single seeds rule two pairs out at every record length: seed 11 (a narrow band on 27 channels) at w2_beta 8 has kappa_a 9e3 ... 9e4,
and seed 9 under if_win at w2_beta 16 has 3.6e5.  Of the offsets 99800 ... 101799, 27 avoid both; put the key alone on three to five
of the 16 draws, among them a ragged multi-shot draw, a gauge draw, a directional draw and a draw with water; leave every keyed mode on
at least two draws; draw every w2_beta (absent, 0.5, 8, 16) at least three times, each at least once under a band-pass and at least
once without one; keep an empty window under if_win; and silence a channel on at least four draws, with and without a band-pass.
99826 is the first of them, and on it every default seed has a target: the key alone on seeds 1, 3, 7, 13; w2_beta absent on 0, 2, 9,
0.5 on 4, 8, 10, 11, 12, 13, 8 on 5, 6, 7, 16 on 1, 3, 14, 15; a silenced channel on 0, 1, 11, 12, 13, 14, 15.  The largest
kappa_a is seed 5's 793 (narrow band, w2_beta 8), near the cap; the next is seed 14's 188.

The dead trace.  The conditioned draw's weights are never 0 and its windows always hold signal, so no trace of a default draw is dead
of itself once the record is live.  In one draw of two the observed data carry ONE silenced channel in the shot of the one-shot call
(exact zeros: A == 0; fuzz_sides.w2_oracle_side) -- the observed gathers are otherwise lame_true's on both builds, and the files are
the conditioned draw's, unchanged.

The water yardstick.  On seed 0 (the sources inside 15 rows of water) the two oracle builds' gMu differ by 1.1e-2 ... 6.5e-2 of the
whole image for every (alone, w2_beta) pair at four times the record, all of it inside the water, where mu is 0 and stays 0; below the water
they agree to 3.8e-5.  fuzz_sides.w2_gradient_spread therefore measures the build yardstick where fuzz_common.gradient_miss has its
teeth (below the water against its floor; the whole image for gLambda and gDen), as the conditioned fuzz leaves hvMu out under water.

The option sets.  A seed's option set is draw_born's, which draw_w2 leaves unchanged: the default 16 seeds hold eight of the ten
BORN_OPTION_SETS -- every family but amu_fly (and of bz the value 1, not 4).  The test asserts exactly that set, so that a change of
either generator shows."""
import hashlib
import json

import numpy as np
import pytest

import cond_gn_ref as G
import fuzz_common as C
import fuzz_draws as D
import w2_held as H
import w2_ref as W
from fuzz_sides import W2_KAPPA_CAP, describe_w2, w2_oracle_side
from test_gpu_w2_data import KEYSETS, problem

SEEDS = C.DEFAULT_SEEDS
W2_RAW_DIGEST = "46e071f6f7e78197715e731287d6fb5cb431ec97228f4a801b52f89c6203bb47"
W2_FILES_DIGEST = "1ab849331ba1a2bee3be7d51e6bd268a5e53becc5a564b0783fd2fa08055d6c5"
FAMILIES = ("default", "batch", "bwd_fuse", "bz", "quiet_skip", "rho_fly", "rk_lazy", "xcd_remap")      # of BORN_OPTION_SETS: all but amu_fly


@pytest.fixture(scope="module")
def sides(oracle, oracle_nvfma, tmp_path_factory):
    """{seed: (w2_oracle_side's dict or None, scale)} of the default seeds, with the re-draw of the GPU test"""
    return C.default_sides(w2_oracle_side, tmp_path_factory.mktemp("w2_fuzz"), oracle, oracle_nvfma)


def test_w2_fuzz_draws_are_what_they_were(sides):
    """What the generator of draw_w2 draws hashes to one digest; the keyed file and its twin at the scale the GPU test takes to another:
    the conditioned file's keys plus the W2 keys (or those alone), the twin the same without them, both on the conditioned survey."""
    raw_digest = hashlib.sha256(json.dumps([D.w2_raw(seed) for seed in SEEDS], sort_keys=True).encode()).hexdigest()
    h = hashlib.sha256()
    skip = ("survey_fname", "data_dir_name", "scratch_dir_name")
    for seed in SEEDS:
        o, scale = sides[seed]
        assert o is not None, seed
        c, w = o["c"], o["w"]
        para, twin, cpara = w["pb"]["para"], w["twin"]["para"], c["pb"]["para"]
        assert para[W.KEY] is True and para.get(W.BETA_KEY, W.BETA) == w["beta"] and (W.BETA_KEY in para) == (w["drawn"] is not None), seed
        assert not any(k in twin or k in cpara for k in D.W2_KEYS), seed
        assert {k: v for k, v in para.items() if k not in D.W2_KEYS + skip} == {k: v for k, v in twin.items() if k not in skip}, seed
        if w["alone"]:
            assert w["mode"] == "alone" and not any(k in para for k in G.COND_KEYS), seed
            assert {k: v for k, v in twin.items() if k not in skip} == {k: v for k, v in cpara.items() if k not in skip + G.COND_KEYS}, seed
        else:
            assert w["mode"] == c["mode"] and {k: v for k, v in twin.items() if k not in skip} == {k: v for k, v in cpara.items() if k not in skip}, seed
        for pb in (w["pb"], w["twin"]):
            assert json.load(open(pb["survey_fname"])) == json.load(open(c["pb"]["survey_fname"])), seed
            assert json.load(open(pb["para_fname"])) == pb["para"], seed
        h.update(json.dumps([seed, scale, w["mode"], w["alone"], w["beta"]]).encode())
        h.update(json.dumps({k: v for k, v in para.items() if k not in skip}, sort_keys=True).encode())
    print("w2 fuzz digests: raw %s, files %s" % (raw_digest, h.hexdigest()))
    assert (raw_digest, h.hexdigest()) == (W2_RAW_DIGEST, W2_FILES_DIGEST)


def test_w2_fuzz_draws_have_targets_and_cover_what_the_fuzz_is_for(sides):
    count = dict(ragged=0, gauge=0, directional=0, scattered=0, water=0, padded=0, oblong=0, alone=0, one_shot_not_0=0, dead_beside_live=0, empty_window=0)
    count.update({m: 0 for m in D.COND_MODES})
    count.update({"beta %r" % x: 0 for x in D.W2_BETAS})
    families, alone_on = set(), dict(ragged=0, gauge=0, directional=0, water=0)
    for seed in SEEDS:
        o, scale = sides[seed]
        assert o is not None and scale <= 4, "seed %d: no live record" % seed
        b, d, w = o["b"], o["d"], o["w"]
        pb, sv = w["pb"], w["pb"]["survey"]
        print("w2 fuzz seed %d (%s): kappa_a %.2f, kappa_W %.2f, build yardsticks %r, smallest tie margin %.2e, the one shot %d of %d"
              % (seed, describe_w2(o, scale), o["kappa_a"], o["kappa_W"], {k: "%.1e" % y for k, y in o["yard"].items()}, o["margin"], o["one"], len(o["live"])))
        assert o["target"] and o["kappa_a"] <= W2_KAPPA_CAP and C.has_target(*o["yard"].values()), (seed, o["kappa_a"], o["yard"])
        assert o["ref"]["misfit"] > 0 and G.norm(o["ref"]["adj"]) > 0, seed
        shots = [sv["shot%d" % i] for i in G.shots_of(pb)]
        assert [int(sh["nrec"]) for sh in shots] == b["counts"] == [a.shape[0] for a in o["ref"]["jv"]], seed
        assert o["live"][o["one"]] and not any(o["live"][o["one"] + 1:]), seed
        if sum(o["live"]) > 1:
            assert o["one"] > 0, seed      # the one-shot call is never on shot 0
        ragged = b["ragged"] and len(shots) > 1
        has = dict(ragged=ragged, gauge=b["G"], directional=any("das_sensitivity" in sh for sh in shots), water=d["water"])
        families.add(sorted(b["opts"])[0] if b["opts"] else "default")
        count[w["mode"]] += 1
        count["beta %r" % w["drawn"]] += 1
        windowed = w["mode"] in ("window", "both")
        for name, on in list(has.items()) + [("scattered", d["kind"] == 2 and not b["G"]), ("padded", pb["nPad"] > 0),
                                             ("oblong", pb["para"]["dz"] != pb["para"]["dx"]), ("one_shot_not_0", o["one"] > 0),
                                             ("dead_beside_live", o["dead_beside_live"]), ("empty_window", windowed and o["c"]["empty"])]:
            count[name] += bool(on)
        if w["alone"]:
            for name in alone_on:
                alone_on[name] += bool(has[name])
    print(count, "the key alone on", alone_on, "option-set families", sorted(families))
    assert all(count["beta %r" % x] >= 3 for x in D.W2_BETAS), count
    assert all(count[m] >= 2 for m in D.COND_MODES), count
    assert 3 <= count["alone"] <= 5 and all(n >= 1 for n in alone_on.values()), (count, alone_on)
    assert count["ragged"] >= 3 and count["gauge"] >= 2 and count["directional"] >= 1 and count["water"] >= 2 and count["scattered"] >= 1, count
    assert count["one_shot_not_0"] >= 2 and count["padded"] >= 1 and count["oblong"] >= 1, count
    assert count["dead_beside_live"] >= 1 and count["empty_window"] >= 1, count
    assert sorted(families) == sorted(FAMILIES), families


# ---- layer A on the CPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(oracle, oracle_nvfma, tmp_path_factory):
    """the cases of tests/test_gpu_w2_kernel_fuzz.py with each oracle build's C in the place of the library's:
    [(what, pb, beta, co, cs per build)]"""
    tmp, out = tmp_path_factory.mktemp("w2_kinds"), []
    for nt in W.FUZZ_NTS:
        for beta in W.FUZZ_BETAS:
            kinds = W.trace_kinds(nt, W.kind_seed(nt, beta))
            for keys in KEYSETS:
                pb = problem(tmp / ("%d_%g_%s" % (nt, beta, keys)), nt, (7,), keys, "w2k", **{W.BETA_KEY: beta})
                cond = [(W.C_of(lib, pb, kinds["obs"], 0), W.C_of(lib, pb, kinds["syn"], 0)) for lib in (oracle, oracle_nvfma)]
                out.append(("nt %d beta %g %s" % (nt, beta, keys), pb, beta, cond))
    return out


def test_every_case_of_the_kernel_fuzz_decides_its_nodes_by_a_margin(cases):
    """kinds 0 to 6 of every case, both oracle builds' C: w2_ref.tie_margin >= 64 nt 2^-53 on every live trace.  Two float64 sums of
    n positive terms in different orders differ by less than n 2^-53 of the sum; F and G are at most 1.  A kind or seed that fails is
    re-seeded (w2_ref.KIND_SEED0), never exempted."""
    smallest = (np.inf, None)
    for what, pb, beta, cond in cases:
        nt = pb["nSteps"]
        for build, (co, cs) in zip(("plain", "nvfma"), cond):
            live = 0
            for r in range(7):
                mg = W.tie_margin(co[r], cs[r], float(pb["para"]["dt"]), beta)
                live += np.isfinite(mg)
                smallest = min(smallest, (mg, "%s channel %d (%s build)" % (what, r, build)))
                assert mg >= W.TIE_FACTOR * nt * 2.0 ** -53, (what, build, r, mg)
            assert live == (6 if "if_win" in pb["para"] else 7), (what, build, live)      # (channel 1 has weight 0 under if_win)
    print("w2 kernel fuzz: the smallest tie margin of %d cases x 2 builds is %.3e, %s; the condition at nt 1025 is %.3e"
          % (len(cases), smallest[0], smallest[1], W.TIE_FACTOR * 1025 * 2.0 ** -53))


WEAKER = {"the tile carry of the suffix sum dropped": dict(tile=256), "A from the synthetic trace": dict(scale_from="syn"),
          "w_r of channel 0 for every channel": dict(first_weight=True), "w2_beta ignored": dict(beta=W.BETA),
          "the projection - sum f psi dropped": dict(project=False)}


def test_the_comparisons_can_fail(oracle, cases):
    """Five weaker references on the cases of layer A (the plain build's C), each measured against the bounds of
    w2_held.on_identical_inputs: the misfit's 8 EPS, and 8 EPS per trace on the window sets or 16 EPS rel-L2 under filter.  Each misses
    by at least 5 x on at least one case (the weight: only under if_win; the carry: only where nt - 1 exceeds a tile; A from syn moves
    the misfit itself)."""
    miss = {name: {} for name in WEAKER}
    for what, pb, beta, cond in cases:
        co, cs = [cond[0][0]], [cond[0][1]]
        ct = lambda a64: [W.Ct_of(oracle, pb, a64[0].astype(np.float32), 0)]
        f_ref, a_ref, _ = W.conditioned_misfit(oracle, pb, co, cs)
        a_ref = [x.astype(np.float64) for x in ct(a_ref)]
        for name, wrong in WEAKER.items():
            f, a, _ = W.conditioned_misfit(oracle, pb, co, cs, **wrong)
            gap_f, worst, gap_l2, _ = H.deviations(f, ct(a), f_ref, a_ref)
            miss[name][what] = max(gap_f / H.MISFIT_EPS, gap_l2 / H.L2_EPS if "filter" in pb["para"] else worst / H.TRACE_EPS)
    for name, by_case in miss.items():
        top = max(by_case, key=by_case.get)
        print("w2 fuzz, a weaker reference (%s): misses a bound by %.2e x on %s; by at least 5 x on %d of %d cases"
              % (name, by_case[top], top, sum(m >= 5.0 for m in by_case.values()), len(by_case)))
    for name, by_case in miss.items():
        assert max(by_case.values()) >= 5.0, (name, by_case)
