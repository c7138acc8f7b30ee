"""The oracle side of tests/test_gpu_conditioned_gn_fuzz.py on its default 16 seeds, on the CPU: what draw_conditioned draws and writes
is held by a digest; every draw has a live record, discriminating inputs and a target at some scale (so no default seed reaches the
xfail branch on the GPU); Z C J d is close to the conditioned residual (cos >= 0.5), which is what makes <g, d> decide something;
between them the draws hold what the fuzz is for; and the comparison can fail -- C in the place of C^T, a forgotten Z, and the windows
and src_weight of shot 0 used for another shot each miss the reference by at least 5 x the tolerance on a default seed.

The generator's offset.  Option set, ragged counts, gauge, water, directional and scattered channels and nSteps belong to draw_problem
and draw_born; draw_conditioned's own generator decides the mode and the empty window.  Under the narrow band the share of |C J v|^2 in
time sample 0 is 8.0e-3 on seed 3 and 6.6e-3 on seed 15, 4.2e-3 on seeds 7 and 10 and below 4e-4 on the others (measured with the mode
forced to "narrow" on every seed), and the windows are live in modes "window" and "both" only.  Of the offsets 98000 ... 98399, 29 give
every mode at least three times, "narrow" on seed 3 or 15, a window mode on two of the ragged multi-shot seeds 0, 2, 3, 6, 7 and an empty
window on two draws whose windows are live; 98035 is the one of them whose empty windows fall on two ragged draws (seeds 0 and 7)."""
import hashlib
import json

import numpy as np
import pytest

import cond_gn_ref as G
import exact_adjoint_ref as X
import fuzz_common as C
import fuzz_draws as D
from fuzz_sides import conditioned_oracle_side, describe_conditioned

SEEDS = C.DEFAULT_SEEDS
TOL = X.TOL
COND_RAW_DIGEST = "dc381a26b6114ab306dbf199a5c594c8fea79edc0a4ed34d26ee54ec38922370"
COND_FILES_DIGEST = "b4d795ebb4f4491a64e698059f050405134b015ffcb9d7b92fe3abc3af7db03c"


@pytest.fixture(scope="module")
def sides(oracle, oracle_nvfma, tmp_path_factory):
    """{seed: (conditioned_oracle_side's dict or None, scale)} of the default seeds, with the re-draw of the GPU test"""
    return C.default_sides(conditioned_oracle_side, tmp_path_factory.mktemp("cond_fuzz"), oracle, oracle_nvfma)


def test_conditioned_fuzz_draws_are_what_they_were(sides):
    """What draw_conditioned draws before it sees a gather (mode, the window draws, the empty window, the seeds of v) hashes to one
    digest; the pair of files it writes at the scale the GPU test takes -- the windows sit on the reference's own arrivals, at whole
    time samples for t10 and t90 -- to another.  The plain files of the draw lose their joint weights and nothing else."""
    h = hashlib.sha256()
    for seed in SEEDS:
        raw = D.conditioned_raw(seed)
        h.update(json.dumps({k: (np.asarray(v).round(12).tolist() if isinstance(v, np.ndarray) else v) for k, v in raw.items()}, sort_keys=True).encode())
    raw_digest = h.hexdigest()
    h = hashlib.sha256()
    for seed in SEEDS:
        o, scale = sides[seed]
        assert o is not None, seed
        c, b, plain = o["c"], o["b"], o["d"]["pb"]["para"]
        assert b["weights"] is None and not any(k.startswith("misfit_w_") or k in G.COND_KEYS for k in plain), seed
        para = c["pb"]["para"]
        assert {k: v for k, v in para.items() if k not in G.COND_KEYS + ("survey_fname", "data_dir_name")} == \
            {k: v for k, v in plain.items() if k not in ("survey_fname", "data_dir_name")}, seed
        h.update(json.dumps([seed, scale, c["mode"], c["empty"]]).encode())
        h.update(json.dumps({k: v for k, v in para.items() if k not in ("survey_fname", "data_dir_name", "scratch_dir_name")}, sort_keys=True).encode())
        sv = json.load(open(c["pb"]["survey_fname"]))
        for k in sorted(sv):
            if k.startswith("shot"):
                sh = dict(sv[k])
                for key in ("win_start", "win_end", "weights"):
                    sh[key] = [float("%.6e" % x) for x in sh[key]]
                sv[k] = sh
        h.update(json.dumps(sv, sort_keys=True).encode())
    print("conditioned fuzz digests: raw %s, files %s" % (raw_digest, h.hexdigest()))
    assert (raw_digest, h.hexdigest()) == (COND_RAW_DIGEST, COND_FILES_DIGEST)


def test_conditioned_fuzz_draws_have_targets_and_cover_what_the_fuzz_is_for(sides):
    count = dict(ragged=0, gauge=0, directional=0, scattered=0, water=0, empty=0, odd=0, narrow_z=0, padded=0, oblong=0)
    count.update({m: 0 for m in D.COND_MODES})
    structures = set()
    for seed in SEEDS:
        o, scale = sides[seed]
        assert o is not None and scale <= 4, "seed %d: no live record with discriminating inputs" % seed
        b, d, c, ref = o["b"], o["d"], o["c"], o["ref"]
        pb, sv = c["pb"], c["pb"]["survey"]
        print("conditioned fuzz seed %d (%s): build spread %r, cond_g %.1e (product %.1e), cos(Z C J d, r) %.3f, sample 0 holds %.1e of |C J v|^2, "
              "|C d| / |d| and |C C d| / |C d| %r" % (seed, describe_conditioned(o, scale), {k: "%.1e" % y for k, y in o["yard"].items()}, o["cond_g"],
                                                   o["gn_cond"], ref["cos_dr"], ref["share0"], {k: "%.3f %.3f" % v for k, v in o["ratios"].items()}))
        assert o["target"], (seed, o["yard"], o["cond_g"], o["gn_cond"])
        assert ref["cos_dr"] >= 0.5, (seed, ref["cos_dr"])
        # the conditions on the inputs
        assert all(abs(r - 1.0) > 0.10 for pair in o["ratios"].values() for r in pair), (seed, o["ratios"])
        shots = [sv["shot%d" % i] for i in G.shots_of(pb)]
        assert [int(sh["nrec"]) for sh in shots] == b["counts"] == [a.shape[0] for a in ref["jv"]], seed
        live_win = c["mode"] in ("window", "both")
        if live_win:
            assert any(len(set(sh["weights"])) > 1 for sh in shots if int(sh["nrec"]) > 1), seed
        assert [sh["src_weight"] for sh in shots] == [0.3 + 0.05 * k for k in range(len(shots))], seed
        T = pb["nSteps"] * float(pb["para"]["dt"])
        for i, sh in enumerate(shots):
            for r_, (t0, t1, w) in enumerate(zip(sh["win_start"], sh["win_end"], sh["weights"])):
                assert 0.0 <= t0 <= t1 <= T * (1 + 1e-12) and 0.5 <= w <= 2.0, (seed, i, r_)
                assert (t0 == t1) == (c["empty"] == (i, r_)), (seed, i, r_)
        assert o["live"][o["one"]] and not any(o["live"][o["one"] + 1:]), seed
        if sum(o["live"]) > 1:
            assert o["one"] > 0, seed      # the one-shot call is never on shot 0
        omega = X.mask_omega(pb)
        for pert in (o["v"], o["dm"]):
            assert all(np.abs(a[omega]).max() > 0 and not np.any(a[~omega]) for a in pert), seed
        directional = any("das_sensitivity" in sh for sh in shots)
        structures.add(json.dumps(b["opts"]))
        count[c["mode"]] += 1
        for name, on in (("ragged", b["ragged"] and len(shots) > 1), ("gauge", b["G"]), ("directional", directional), ("scattered", d["kind"] == 2 and not b["G"]),
                         ("water", d["water"]), ("empty", c["empty"] and live_win), ("odd", pb["nSteps"] % 2), ("padded", pb["nPad"] > 0),
                         ("oblong", pb["para"]["dz"] != pb["para"]["dx"]), ("narrow_z", c["mode"] == "narrow" and ref["share0"] >= 5.0 * TOL)):
            count[name] += bool(on)
    print(count, len(structures))
    assert all(count[m] >= 2 for m in D.COND_MODES), count
    assert count["ragged"] >= 3 and count["gauge"] >= 2 and count["directional"] >= 1 and count["scattered"] >= 1 and count["water"] >= 2, count
    assert count["empty"] >= 1 and count["odd"] >= 1 and count["narrow_z"] >= 1 and count["padded"] >= 1 and count["oblong"] >= 1, count
    assert len(structures) >= 4, structures


def test_the_comparisons_can_fail(oracle, sides):
    """Three weaker passes, on the reference side, on the scales of the GPU test: C in the place of C^T misses <d, H v> on a "both" draw
    (<C Z C J v, J d> against the reference); without Z, v^T H v is off on the narrow draw whose sample 0 carries weight; with the
    windows and src_weight of shot 0, v^T H_k v of the one-shot call is off on a ragged draw whose windows are live."""
    miss = dict(transpose={}, z={}, shot0={})
    for seed in SEEDS:
        o, scale = sides[seed]
        if o is None:
            continue
        c, ref, k = o["c"], o["ref"], o["one"]
        pb = c["pb"]
        if c["mode"] == "both":
            r, _, s = o["cmp"]["<d,Hv>"]
            miss["transpose"][seed] = abs(G.dot(G.C_all(oracle, pb, ref["zv"]), ref["jd"]) - r) / s
        if c["mode"] == "narrow":
            r, _, s = o["cmp"]["vHv"]
            miss["z"][seed] = abs(G.dot(ref["cjv"], ref["cjv"]) - r) / s
        if o["b"]["ragged"] and k > 0 and c["mode"] in ("window", "both"):
            ids = G.shots_of(pb)
            sv = dict(pb["survey"])
            sh, sh0 = dict(sv["shot%d" % ids[k]]), sv["shot%d" % ids[0]]
            n = int(sh["nrec"])
            for key in ("win_start", "win_end", "weights"):      # shot 0's table from its first entry on, as a wrong offset reads it
                sh[key] = (sh0[key] + sh[key])[:n]
            sh["src_weight"] = sh0["src_weight"]
            sv["shot%d" % ids[k]] = sh
            wrong = G.Z(G.C_of(oracle, dict(pb, survey=sv), ref["jv"][k], ids[k]))
            r, _, s = o["cmp"]["vHv one shot"]
            miss["shot0"][seed] = abs(G.dot([wrong], [wrong]) - r) / s
    for what, by_seed in miss.items():
        print("conditioned fuzz, a weaker pass (%s): misses by %r of the scale" % (what, {s: "%.2e" % m for s, m in by_seed.items()}))
        assert by_seed and max(by_seed.values()) >= 5.0 * TOL, (what, by_seed)
