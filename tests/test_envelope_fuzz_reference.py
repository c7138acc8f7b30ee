"""The oracle side of tests/test_gpu_envelope_fuzz.py on its default 16 seeds, on the CPU: what draw_envelope draws and writes is held
by a digest; every draw has a live record and a target at some scale (so no default seed reaches the xfail branch on the GPU);
Z D C J d is not orthogonal to rho, which is what makes <g, d> decide something; between them the draws hold what the fuzz is for; the
inputs discriminate (the L2 quantities in the place of the envelope's miss on every seed, D at C obs instead of C syn misses the cross
term); and the comparisons can fail -- five weaker passes built on the reference side each miss a comparison of the GPU test by at
least 5 x its tolerance on a default seed.

The cosine.  cos(Z D C J d, rho) is at least 0.95 on 15 seeds and 0.457 on seed 5 (two shots, 13 channels, the narrow band: the
envelope's residual there is dominated by a part that the model difference d does not explain to first order).  The bound is 0.4
(fuzz_sides.ENV_COS), where the L2 side asks 0.5: <g, d> is compared on the scale |<g, d>| itself, so what it needs is that the
projection is not a cancellation residue, and 0.4 of |Z D C J d| |rho| is as far from one as 0.5 is.

The generator's offset.  The mode of a seed belongs to draw_conditioned (filter: seeds 1, 2, 15; narrow: 3, 5, 11; window: 7, 9, 14;
both: the other seven); draw_envelope's own generator only decides which draws lose their conditioning keys.  Of the offsets
99000 ... 99399, 66 strip the keys on three to five of the 16 draws, leave every keyed mode at least twice, and put the key alone on a
ragged multi-shot draw (seeds 0, 2, 3, 6, 7), a gauge draw (3, 7, 9, 10, 12), a directional draw (0, 8, 13, 15) and a draw with water
(0, 10, 12, 13, 14, 15); 99001 is the first of them (the key alone on seeds 0, 1 and 12)."""
import hashlib
import json

import numpy as np
import pytest

import cond_gn_ref as G
import envelope_ref as E
import fuzz_common as C
import fuzz_draws as D
import gauge_ref as GA
from fuzz_sides import ENV_COS, describe_envelope, envelope_build_side, envelope_oracle_side, oracle_gathers

SEEDS = C.DEFAULT_SEEDS
ENV_RAW_DIGEST = "9d4a47756be3bbc9c1bacc713d574463e95a3b4d2d8f78439886059f051c3c5e"
ENV_FILES_DIGEST = "86fd3055a24b7fc6d0c88ccb826d13623da86d2c5070f085f8f55937bf1d7a1e"
KEYED = D.COND_MODES


@pytest.fixture(scope="module")
def sides(oracle, oracle_nvfma, tmp_path_factory):
    """{seed: (envelope_oracle_side's dict or None, scale)} of the default seeds, with the re-draw of the GPU test"""
    return C.default_sides(envelope_oracle_side, tmp_path_factory.mktemp("env_fuzz"), oracle, oracle_nvfma)


def tol(o, key, nominal=C.GRAD_TOL):
    """the relative tolerance of a comparison of the GPU test: nominal + cond_env + 3 x the two builds' difference"""
    return nominal + o["cond_env"] + C.YARD * o["yard"][key]


def test_envelope_fuzz_draws_are_what_they_were(sides):
    """What the generator of draw_envelope draws hashes to one digest; the keyed file and its twin at the scale the GPU test takes to
    another: the conditioned file's keys plus the key (or the key alone), the twin the same without it, both on the conditioned survey."""
    raw_digest = hashlib.sha256(json.dumps([D.envelope_raw(seed) for seed in SEEDS], sort_keys=True).encode()).hexdigest()
    h = hashlib.sha256()
    skip = ("survey_fname", "data_dir_name", "scratch_dir_name")
    for seed in SEEDS:
        o, scale = sides[seed]
        assert o is not None, seed
        c, e = o["c"], o["e"]
        para, twin, cpara = e["pb"]["para"], e["twin"]["para"], c["pb"]["para"]
        assert para.get(D.ENV_KEY) is True and D.ENV_KEY not in twin and D.ENV_KEY not in cpara, seed
        assert {k: v for k, v in para.items() if k != D.ENV_KEY and k not in skip} == {k: v for k, v in twin.items() if k not in skip}, seed
        if e["alone"]:
            assert e["mode"] == "alone" and not any(k in para for k in G.COND_KEYS), seed
            assert {k: v for k, v in twin.items() if k not in skip} == {k: v for k, v in cpara.items() if k not in skip + G.COND_KEYS}, seed
        else:
            assert e["mode"] == c["mode"] and {k: v for k, v in twin.items() if k not in skip} == {k: v for k, v in cpara.items() if k not in skip}, seed
        for pb in (e["pb"], e["twin"]):
            assert json.load(open(pb["survey_fname"])) == json.load(open(c["pb"]["survey_fname"])), seed
            assert json.load(open(pb["para_fname"])) == pb["para"], seed
        h.update(json.dumps([seed, scale, e["mode"], e["alone"]]).encode())
        h.update(json.dumps({k: v for k, v in para.items() if k not in skip}, sort_keys=True).encode())
    print("envelope fuzz digests: raw %s, files %s" % (raw_digest, h.hexdigest()))
    assert (raw_digest, h.hexdigest()) == (ENV_RAW_DIGEST, ENV_FILES_DIGEST)


def test_envelope_fuzz_draws_have_targets_and_cover_what_the_fuzz_is_for(sides):
    count = dict(ragged=0, gauge=0, directional=0, scattered=0, water=0, alone=0, padded=0, oblong=0, plans=0)
    count.update({m: 0 for m in KEYED})
    structures = set()
    for seed in SEEDS:
        o, scale = sides[seed]
        assert o is not None and scale <= 4, "seed %d: no live record" % seed
        b, d, e, ref = o["b"], o["d"], o["e"], o["ref"]
        pb, sv = e["pb"], e["pb"]["survey"]
        print("envelope fuzz seed %d (%s): build spread %r, cond_env %.1e, cos(Z D C J d, rho) %.3f, the one shot %d of %d, peak |syn| %.1e, weakest channel's peak %.1e"
              % (seed, describe_envelope(o, scale), {k: "%.1e" % y for k, y in o["yard"].items()}, o["cond_env"], ref["cos_dr"], o["one"], len(ref["syn"]),
                 max(float(np.abs(s).max()) for s in ref["syn"]), min(float(np.abs(s).max(axis=1).min()) for s in ref["syn"])))
        assert o["target"], (seed, o["yard"], o["cond_env"])
        assert o["cond_env"] <= C.TARGET_CAP and ref["cos_dr"] >= ENV_COS, (seed, o["cond_env"], ref["cos_dr"])
        shots = [sv["shot%d" % i] for i in G.shots_of(pb)]
        assert [int(sh["nrec"]) for sh in shots] == b["counts"] == [a.shape[0] for a in ref["jv"]], seed
        assert o["live"][o["one"]] and not any(o["live"][o["one"] + 1:]), seed
        if sum(o["live"]) > 1:
            assert o["one"] > 0, seed      # the one-shot call is never on shot 0
        ragged = b["ragged"] and len(shots) > 1
        structures.add(json.dumps(b["opts"]))
        count[e["mode"]] += 1
        for name, on in (("ragged", ragged), ("gauge", b["G"]), ("directional", any("das_sensitivity" in sh for sh in shots)),
                         ("scattered", d["kind"] == 2 and not b["G"]), ("water", d["water"]), ("padded", pb["nPad"] > 0),
                         ("oblong", pb["para"]["dz"] != pb["para"]["dx"]), ("plans", ragged and len(set(b["counts"])) > 1 and o["one"] > 0)):
            count[name] += bool(on)
    print(count, len(structures))
    assert all(count[m] >= 2 for m in KEYED + ("alone",)), count
    assert count["ragged"] >= 3 and count["gauge"] >= 2 and count["directional"] >= 1 and count["water"] >= 2, count
    assert count["plans"] >= 2 and count["padded"] >= 1 and count["oblong"] >= 1 and len(structures) >= 4, (count, structures)


def test_the_inputs_discriminate(oracle, sides):
    """The L2 misfit 1/2 |Z (C obs - C syn)|^2 and |Z C J v|^2 in the place of the envelope's miss by at least 5 x the tolerance on EVERY
    seed (a pass that ignores the key cannot go unnoticed anywhere); D taken at C obs instead of C syn misses the cross term on at least
    one."""
    at_obs = {}
    for seed in SEEDS:
        o, _ = sides[seed]
        pb, ref = o["e"]["pb"], o["ref"]
        c = lambda gs: [E.C_of(oracle, pb, g, sid) for g, sid in zip(gs, G.shots_of(pb))]
        r = [E.Z(a.astype(np.float64) - s) for a, s in zip(c(ref["obs"]), c(ref["syn"]))]
        zv = [E.Z(a) for a in c(ref["jv"])]
        miss_m = abs(0.5 * G.dot(r, r) - ref["misfit"]) / ref["misfit"]
        miss_v = abs(G.dot(zv, zv) - ref["nv"]) / ref["nv"]
        wrong = envelope_build_side(oracle, pb, o["raw"], o["one"], bg=ref["obs"])
        _, _, s = o["cmp"]["<d,Hv>"]
        at_obs[seed] = abs(wrong["cross"] - ref["cross"]) / s / tol(o, "<d,Hv>")
        print("envelope fuzz seed %d: the L2 misfit misses by %.2e of the envelope's (tolerance %.1e), |Z C J v|^2 by %.2e of |Z D C J v|^2 (%.1e); "
              "D at C obs misses the cross term by %.1f x its tolerance" % (seed, miss_m, tol(o, "misfit", C.MISFIT_TOL), miss_v, tol(o, "vHv"), at_obs[seed]))
        assert miss_m >= 5.0 * (C.MISFIT_TOL + 2.0 * o["cond_env"] + C.YARD * o["yard"]["misfit"]) and miss_v >= 5.0 * tol(o, "vHv"), seed
    assert max(at_obs.values()) >= 5.0, at_obs


def test_the_comparisons_can_fail(oracle, sides):
    """Five weaker passes on the reference side, each measured on the scale and against the tolerance of the GPU test's comparison:
      gauge        the background gather is the centre member's, no gauge average: v^T H v on a gauge draw
      directional  it ignores das_sensitivity: v^T H v on a directional draw
      shot 0       the one-shot call's D at shot 0's background gather (its first nrec_k channels, repeated where it has fewer):
                   v^T H_k v on a ragged draw whose one shot is not shot 0
      hilbert      the H((H s) w) half of D^T dropped: v^T H v (= <2 s C J v, Z D C J v> then) on every draw
      z            Z dropped: v^T H v = |D C J v|^2
    -> each misses by at least 5 x the tolerance on at least one default seed."""
    miss = dict(gauge={}, directional={}, shot0={}, hilbert={}, z={})
    for seed in SEEDS:
        o, _ = sides[seed]
        d, b, e, ref, raw, k = o["d"], o["b"], o["e"], o["ref"], o["raw"], o["one"]
        pb, plain, sv = e["pb"], d["pb"], e["pb"]["survey"]
        ids = G.shots_of(pb)
        r, _, s = o["cmp"]["vHv"]
        rel = lambda got, key="vHv": abs(got - o["cmp"][key][0]) / o["cmp"][key][2] / tol(o, key)
        if b["G"]:
            centre = [GA.centre_of(a[3][None], b["G"])[0] for a in raw["raw"]["syn"]]
            miss["gauge"][seed] = rel(envelope_build_side(oracle, pb, raw, k, bg=centre)["nv"])
        if any("das_sensitivity" in sv["shot%d" % i] for i in ids):
            bare = {key: ({q: val for q, val in sh.items() if q != "das_sensitivity"} if GA.is_shot(key) else sh) for key, sh in d["sv"].items()}
            blind = [np.ascontiguousarray(g[3], dtype=np.float32) for g in oracle_gathers(oracle, o["m"], plain["Stf"].numpy(), np.asarray(ids, np.int32), plain["para"], bare)]
            miss["directional"][seed] = rel(envelope_build_side(oracle, pb, raw, k, bg=blind)["nv"])
        if b["ragged"] and k > 0 and "vHv one shot" in o["cmp"]:
            shot0 = np.resize(ref["syn"][0], ref["syn"][k].shape)      # rows of shot 0, repeated cyclically where it has fewer
            miss["shot0"][seed] = rel(envelope_build_side(oracle, pb, raw, k, syn_one=shot0)["nv_one"], "vHv one shot")
        cs = [E.C_of(oracle, pb, g, i).astype(np.float64) for g, i in zip(ref["syn"], ids)]
        cj = [E.C_of(oracle, pb, g, i).astype(np.float64) for g, i in zip(ref["jv"], ids)]
        miss["hilbert"][seed] = rel(G.dot([2.0 * a * x for a, x in zip(cs, cj)], ref["zv"]))
        full = [E.D(a, x) for a, x in zip(cs, cj)]
        miss["z"][seed] = rel(G.dot(full, full))
    for what, by_seed in miss.items():
        print("envelope fuzz, a weaker pass (%s): misses by %r x the tolerance" % (what, {s: "%.2e" % m for s, m in by_seed.items()}))
    for what, by_seed in miss.items():
        assert by_seed and max(by_seed.values()) >= 5.0, (what, by_seed)
