"""The oracle side of tests/test_gpu_robust_fuzz.py on its default 16 seeds, on the CPU: what draw_robust draws and writes is held by
a digest; every draw has a live record and a target at some scale (so no default seed reaches the xfail branch on the GPU) and tests
both branches of the penalty; between them the draws hold what the fuzz is for; and the comparisons can fail -- five weaker passes built
on the reference side each miss a comparison of the GPU test by at least 5 x its tolerance on a default seed.

The cosine.  cos(Z C J d, psi) is at least 0.65 on seeds 3, 4, 5, 10 and 14 (the keys alone, or if_win without a filter, at a quantile
below 1: the spikes are clipped to delta A, a fraction of the trace's peak, and psi is the clean residual elsewhere).  On the other
eleven (0, 1, 2, 6, 7, 8, 9, 11, 12, 13, 15) it lies between -0.30 and 0.19: under a filter the band-pass spreads each spike of 100 x
the peak over the record, at q = 0.99 and 1.0 A and with it the threshold are of the spikes' size, and psi is then the spikes' residual,
of which the model difference d explains nothing.  There <g, d> = -<Z C J d, psi> is a small projection of two large vectors, and it is
compared on the scale |Z C J d| |psi| (fuzz_sides.robust_oracle_side: ROB_COS = 0.4, the envelope side's bound, decides which scale) --
as strict as the definition allows: a float32 pass can hold a projection to 1e-3 of the product of the norms, not to 1e-3 of what is
left after cancellation.  The exact gradient is still held by the other comparisons of those seeds (the reference-style gradient, the
adjoint source per gather, v^T H v).

The generator's offset.  The mode of a seed belongs to draw_conditioned (filter: seeds 1, 2, 15; narrow: 3, 5, 11; window: 7, 9, 14;
both: the other seven); draw_robust's own generator decides the penalty, robust_delta, robust_quantile, the spikes' seed and which
draws lose their conditioning keys.  Of the offsets 99400 ... 99799, 83 give both penalties and both deltas at least four times each
and every quantile at least three times, strip the keys on three to five of the 16 draws, and put the keys alone on a ragged multi-shot
draw (seeds 0, 2, 3, 6, 7), a gauge draw (3, 7, 9, 10, 12), a directional draw (0, 8, 13, 15) and a draw with water (0, 10, 12, 13, 14,
15); 99411 is the first of them: the keys alone on seeds 3 (ragged, gauge), 4, 5, 8 (directional) and 10 (gauge, water; four shots);
huber on 4, 7, 8, 9, 11, 14, 15; delta 0.1 on 2, 3, 4, 6, 9, 12, 14; the quantile absent on 0, 3, 4, 5, 10, 14, 0.99 on 6, 8, 11, 15,
1.0 on 1, 2, 7, 9, 12, 13.  Seed 14 (if_win alone, 212 traces) has 211 dead traces at the default and steps up to 0.99, where 38 are
dead beside 174 live ones; seed 10 has six channels that the wave never reaches beside 38 live ones."""
import hashlib
import json

import numpy as np
import pytest

import cond_gn_ref as G
import fuzz_common as C
import fuzz_draws as D
import robust_ref as R
from fuzz_sides import ROB_COS, ROB_SHARE, describe_robust, robust_build_side, robust_oracle_side

SEEDS = C.DEFAULT_SEEDS
ROB_RAW_DIGEST = "b6c1f1a99678d15ee5e7aab2c745b85a65607789879888ded7c464badbe12b47"
ROB_FILES_DIGEST = "8e3057f6e3e1522c42f2cd237d17421250eb954a65031798ec5e5ec47dd931f8"
COND = {"vHv": "p", "<d,Hv>": "p", "vHv one shot": "p", "misfit": "m", "<g,d>": "a"}


@pytest.fixture(scope="module")
def sides(oracle, oracle_nvfma, tmp_path_factory):
    """{seed: (robust_oracle_side's dict or None, scale)} of the default seeds, with the re-draw of the GPU test"""
    return C.default_sides(robust_oracle_side, tmp_path_factory.mktemp("rob_fuzz"), oracle, oracle_nvfma)


def tol(o, key):
    """the relative tolerance of a comparison of the GPU test: nominal + the penalty's conditioning term + 3 x the two builds' difference"""
    return (C.MISFIT_TOL if key == "misfit" else C.GRAD_TOL) + o["cond"][COND[key]] + C.YARD * o["yard"][key]


def test_robust_fuzz_draws_are_what_they_were(sides):
    """What the generator of draw_robust draws hashes to one digest; the keyed file and its twin at the scale and the quantile the GPU
    test takes to another: the conditioned file's keys plus the robust keys (or those alone), the twin the same without them, both on the
    conditioned survey."""
    raw_digest = hashlib.sha256(json.dumps([D.robust_raw(seed) for seed in SEEDS], sort_keys=True).encode()).hexdigest()
    h = hashlib.sha256()
    skip = ("survey_fname", "data_dir_name", "scratch_dir_name")
    for seed in SEEDS:
        o, scale = sides[seed]
        assert o is not None, seed
        c, r = o["c"], o["r"]
        para, twin, cpara = r["pb"]["para"], r["twin"]["para"], c["pb"]["para"]
        assert para[R.KEY] == r["kind"] and para[R.DELTA_KEY] == r["delta"] and para.get(R.Q_KEY, R.QUANTILE) == r["quantile"], seed
        assert (R.Q_KEY in para) == (r["drawn"] is not None or r["stepped"]), seed
        assert not any(k in twin or k in cpara for k in R.KEYS), seed
        assert {k: v for k, v in para.items() if k not in R.KEYS + skip} == {k: v for k, v in twin.items() if k not in skip}, seed
        if r["alone"]:
            assert r["mode"] == "alone" and not any(k in para for k in G.COND_KEYS), seed
            assert {k: v for k, v in twin.items() if k not in skip} == {k: v for k, v in cpara.items() if k not in skip + G.COND_KEYS}, seed
        else:
            assert r["mode"] == c["mode"] and {k: v for k, v in twin.items() if k not in skip} == {k: v for k, v in cpara.items() if k not in skip}, seed
        for pb in (r["pb"], r["twin"]):
            assert json.load(open(pb["survey_fname"])) == json.load(open(c["pb"]["survey_fname"])), seed
            assert json.load(open(pb["para_fname"])) == pb["para"], seed
        h.update(json.dumps([seed, scale, r["mode"], r["alone"], r["kind"], r["delta"], r["quantile"], r["stepped"]]).encode())
        h.update(json.dumps({k: v for k, v in para.items() if k not in skip}, sort_keys=True).encode())
    print("robust fuzz digests: raw %s, files %s" % (raw_digest, h.hexdigest()))
    assert (raw_digest, h.hexdigest()) == (ROB_RAW_DIGEST, ROB_FILES_DIGEST)


def test_robust_fuzz_draws_have_targets_and_cover_what_the_fuzz_is_for(sides):
    count = dict(ragged=0, gauge=0, directional=0, scattered=0, water=0, padded=0, oblong=0, alone=0, plans=0, stepped=0, dead_beside_live=0,
                 dead_in_a_window=0, empty_window=0, low_cosine=0)
    count.update({m: 0 for m in D.COND_MODES})
    count.update({k: 0 for k in D.ROB_KINDS})
    count.update({"delta %g" % x: 0 for x in D.ROB_DELTAS})
    count.update({"drawn quantile %r" % q: 0 for q in D.ROB_QUANTILES})
    count.update({"quantile %g" % q: 0 for q in D.ROB_STEPS})
    structures, alone_on = set(), dict(ragged=0, gauge=0, directional=0, water=0)
    for seed in SEEDS:
        o, scale = sides[seed]
        assert o is not None and scale <= 4, "seed %d: no live record" % seed
        b, d, r, ref, cr = o["b"], o["d"], o["r"], o["ref"], o["cond"]
        pb, sv = r["pb"], r["pb"]["survey"]
        print("robust fuzz seed %d (%s): build spread %r, cond a / m / p %.1e / %.1e / %.1e, cos(Z C J d, psi) %.3f, the one shot %d of %d, dead share %.3f, inside the threshold %.3f"
              % (seed, describe_robust(o, scale), {k: "%.1e" % y for k, y in o["yard"].items()}, cr["a"], cr["m"], cr["p"], ref["cos_dr"], o["one"],
                 len(ref["syn"]), o["dead_share"], ref["inside"]))
        assert o["target"], (seed, o["yard"], cr)
        assert max(cr.values()) <= C.TARGET_CAP and ref["outside"] >= ROB_SHARE and ref["inside"] >= ROB_SHARE, (seed, cr, ref["outside"], ref["inside"])
        # <g, d> on its own scale where the cosine allows it, else on the product of the norms (module docstring)
        assert o["cmp"]["<g,d>"][2] == (abs(ref["gd"]) if ref["cos_dr"] >= ROB_COS else ref["gd_norms"]), seed
        assert r["quantile"] == 1.0 or 2 * ref["dead"] <= ref["traces"], (seed, ref["dead"], ref["traces"])
        # every live trace carries a spike, no dead one does
        assert all((idx.size > 0) == (A > 0.0) for (where, _), As in zip(o["plan"], ref["A"]) for idx, A in zip(where, As)), seed
        shots = [sv["shot%d" % i] for i in G.shots_of(pb)]
        assert [int(sh["nrec"]) for sh in shots] == b["counts"] == [a.shape[0] for a in ref["jv"]], seed
        assert o["live"][o["one"]] and not any(o["live"][o["one"] + 1:]), seed
        if sum(o["live"]) > 1:
            assert o["one"] > 0, seed      # the one-shot call is never on shot 0
        ragged = b["ragged"] and len(shots) > 1
        has = dict(ragged=ragged, gauge=b["G"], directional=any("das_sensitivity" in sh for sh in shots), water=d["water"])
        structures.add(json.dumps(b["opts"]))
        count[r["mode"]] += 1
        count[r["kind"]] += 1
        count["delta %g" % r["delta"]] += 1
        count["drawn quantile %r" % r["drawn"]] += 1
        count["quantile %g" % r["quantile"]] += 1
        windowed = r["mode"] in ("window", "both")
        for name, on in list(has.items()) + [("scattered", d["kind"] == 2 and not b["G"]), ("padded", pb["nPad"] > 0),
                                             ("oblong", pb["para"]["dz"] != pb["para"]["dx"]), ("plans", ragged and len(set(b["counts"])) > 1 and o["one"] > 0),
                                             ("stepped", r["stepped"]), ("dead_beside_live", ref["dead_beside_live"]),
                                             ("dead_in_a_window", ref["dead_beside_live"] and r["mode"] == "window"),
                                             ("empty_window", windowed and o["c"]["empty"]), ("low_cosine", ref["cos_dr"] < ROB_COS)]:
            count[name] += bool(on)
        if r["alone"]:
            for name in alone_on:
                alone_on[name] += bool(has[name])
    print(count, "the keys alone on", alone_on, "option sets", sorted(structures))
    assert all(count[k] >= 4 for k in D.ROB_KINDS) and all(count["delta %g" % x] >= 4 for x in D.ROB_DELTAS), count
    assert all(count["drawn quantile %r" % q] >= 3 for q in D.ROB_QUANTILES), count
    assert 3 <= count["alone"] <= 5 and all(n >= 1 for n in alone_on.values()), (count, alone_on)
    assert count["ragged"] >= 3 and count["gauge"] >= 2 and count["directional"] >= 1 and count["water"] >= 2 and count["scattered"] >= 1, count
    assert count["plans"] >= 2 and count["padded"] >= 1 and count["oblong"] >= 1 and len(structures) >= 4, (count, structures)
    assert count["dead_beside_live"] >= 2 and count["dead_in_a_window"] >= 1 and count["empty_window"] >= 2 and count["stepped"] >= 1, count
    assert sum(count[m] for m in ("filter", "both", "narrow")) >= 4 and count["window"] >= 2, count


def next_rank(o, s):
    """a trace whose order statistic k is the observed trace's of rank k + 1 (the largest stays the largest)"""
    v = np.sort(np.abs(np.asarray(o)[1:]))
    return np.concatenate([[0.0], v[1:], v[-1:]]).astype(np.float32)


def test_the_comparisons_can_fail(oracle, sides):
    """Five weaker passes on the reference side, each measured on the scale and against the tolerance of the GPU test's comparison (the
    larger of the misfit's and v^T H v's where both are named):
      A from syn     the scale A from the synthetic trace (robust_ref.trace_parts(scale_from=)): the misfit, v^T H v
      rank k + 1     A the next order statistic: the misfit, v^T H v (no change at q = 1.0, where k is the last rank)
      L2             the L2 quantities 1/2 |Z (C obs - C syn)|^2 and |Z C J v|^2 in the place of the penalty's: a pass that ignores the keys
      shot 0         the weight of the one-shot call taken at shot 0's observed gather (its first nrec_k channels, repeated where it
                     has fewer) -- the store's offset error: v^T H_k v on a draw whose one shot is not shot 0
      w at obs - Jv  the weight at (C obs, C obs - C J v) in the place of (C obs, C syn): v^T H v
    -> each misses by at least 5 x the tolerance on at least one default seed; the L2 quantities on EVERY seed (the misfit everywhere;
    at q = 1.0 under if_win, seeds 7 and 9, the threshold is 50 resp. 10 x the trace's peak, every clean sample lies inside it and
    the PRODUCT is the L2 one to 1e-3 resp. 5e-3 -- the definition at that quantile, not a gap of the draw)."""
    miss = {"A from syn": {}, "rank k + 1": {}, "L2": {}, "shot 0": {}, "w at obs - Jv": {}}
    for seed in SEEDS:
        o, _ = sides[seed]
        r, ref, raw, k = o["r"], o["ref"], o["raw"], o["one"]
        pb, obs = r["pb"], ref["obs"]
        rel = lambda got, key: abs(got - o["cmp"][key][0]) / o["cmp"][key][2] / tol(o, key)
        both = lambda side: max(rel(side["misfit"], "misfit"), rel(side["nv"], "vHv"))
        miss["A from syn"][seed] = both(robust_build_side(oracle, pb, raw, k, obs, scale_from=lambda a, s: s))
        miss["rank k + 1"][seed] = both(robust_build_side(oracle, pb, raw, k, obs, scale_from=next_rank))
        miss["L2"][seed] = max(rel(side[q], key) for side in [robust_build_side(oracle, pb, raw, k, obs, l2=True)] for q, key in (("misfit", "misfit"), ("nv", "vHv")))
        if k > 0 and "vHv one shot" in o["cmp"]:
            shot0 = np.resize(obs[0], obs[k].shape)      # rows of shot 0, repeated cyclically where it has fewer
            miss["shot 0"][seed] = rel(robust_build_side(oracle, pb, raw, k, obs, obs_one=shot0)["nv_one"], "vHv one shot")
        at_jv = [(a.astype(np.float64) - j).astype(np.float32) for a, j in zip(obs, ref["jv"])]
        miss["w at obs - Jv"][seed] = rel(robust_build_side(oracle, pb, raw, k, obs, wsyn=at_jv)["nv"], "vHv")
    for what, by_seed in miss.items():
        print("robust fuzz, a weaker pass (%s): misses by %r x the tolerance" % (what, {s: "%.2e" % m for s, m in by_seed.items()}))
    for what, by_seed in miss.items():
        assert by_seed and max(by_seed.values()) >= 5.0, (what, by_seed)
    assert min(miss["L2"].values()) >= 5.0, miss["L2"]
