"""The oracle side of tests/test_gpu_born_fuzz.py on its default 16 seeds, on the CPU: every draw has a live record at some scale and a
parity target for the Gauss-Newton product (so no default seed reaches the xfail branch on the GPU), born_ref on every draw is the
derivative of the oracle's gathers, and what draw_born draws is held by a digest.

born_ref against the central finite difference (d(m + eps v) - d(m - eps v)) / 2 eps of oracle.cufd(calc_id 2) on the draw's own
channels (the member channels of a gauge draw), rel-L2 per component over all shots, best of eps in {1, 0.1}; the bound is 1e-2, the
discrimination threshold of tests/test_born_reference.py (a dropped coupling term is >= 0.35).  Measured per seed (vx, vz, ett):
   0  1.0e-4 8.0e-5 9.4e-5 |  1  1.4e-4 8.5e-5 1.8e-4 |  2  1.3e-4 1.5e-4 1.4e-4 |  3  4.3e-5 7.4e-5 1.2e-4
   4  1.6e-4 2.4e-4 1.7e-4 |  5  2.3e-4 1.3e-4 2.4e-4 |  6  1.6e-4 1.2e-4 2.9e-4 |  7  4.6e-5 4.4e-5 6.4e-5
   8  1.2e-4 6.1e-5 8.1e-5 |  9  1.3e-4 1.1e-4 1.4e-4 | 10  7.4e-5 8.9e-5 9.0e-5 | 11  1.7e-4 2.7e-4 2.2e-4
  12  7.3e-5 1.1e-4 2.5e-4 | 13  1.6e-4 1.2e-4 1.5e-4 | 14  1.1e-4 7.4e-5 2.0e-4 | 15  9.8e-5 7.4e-5 8.5e-5
The two oracle builds differ by at most 2.6e-4 (seed 12, a vertical gauge below 20 rows of water) of the gradient at obs = syn - J v, the conditioning term is at most 2.5e-5."""
import hashlib
import json

import numpy as np
import pytest

import fuzz_common as C
import fuzz_draws as D
import gauge_ref as GA
from born_ref import COMPS, ROW
from fuzz_sides import born_oracle_side, describe_born, oracle_gathers

SEEDS = C.DEFAULT_SEEDS
BORN_DRAWS_DIGEST = "c54b6efe1fb3f38bc775ebbcf0fd200daaa07f2beeb47d82890dd3972ed3463f"


def test_born_fuzz_draws_are_what_they_were(tmp_path, monkeypatch):
    """What draw_born adds to the first 16 draws -- options, channel counts, weights, gauge, the conditioned twin -- and the two files it
    rewrites hash to the digest taken when the generator was written: a change of the generator is visible."""
    for v in C.ENV:
        monkeypatch.delenv(v, raising=False)
    h = hashlib.sha256()
    for seed in SEEDS:
        d = D.draw_problem(tmp_path / ("s%d" % seed), seed, 1)
        b = D.draw_born(d, seed)
        h.update(json.dumps(dict(b, cond_fname=bool(b["cond_fname"])), sort_keys=True).encode())
        h.update(json.dumps({k: v for k, v in d["pb"]["para"].items() if k not in ("survey_fname", "data_dir_name", "scratch_dir_name")}, sort_keys=True).encode())
        h.update(json.dumps(json.load(open(d["pb"]["survey_fname"])), sort_keys=True).encode())
    assert h.hexdigest() == BORN_DRAWS_DIGEST


@pytest.fixture(scope="module")
def sides(oracle, oracle_nvfma, tmp_path_factory):
    """{seed: (born_oracle_side's dict or None, scale)} of the default seeds, with the re-draw of the GPU test"""
    return C.default_sides(born_oracle_side, tmp_path_factory.mktemp("born_fuzz"), oracle, oracle_nvfma)


def test_born_fuzz_draws_have_parity_targets(sides):
    """NONE of the default seeds lacks a live record or a parity target for the product, and between them the 16 draws hold what the
    fuzz is for: dz != dx, a water layer, ragged channel counts with a single-channel shot, joint weights, a gauge length, a
    conditioned twin, directional channels, and more than one kernel structure."""
    seen, structures = set(), set()
    for seed in SEEDS:
        o, scale = sides[seed]
        assert o is not None, "seed %d: the wave does not reach the channels" % seed
        b, d = o["b"], o["d"]
        print("born fuzz seed %d (%s): build spread %.1e, cond_g %.1e, oracle v^T H v / |W^1/2 J v|^2 %.4f" % (seed, describe_born(o, scale), o["noise_rel"], o["cond_g"], o["ratio"]))
        assert o["target"], (seed, o["noise_rel"], o["cond_g"])
        para = d["pb"]["para"]
        assert not any(k in para for k in GA.COND_KEYS), seed
        if d["water"]:
            assert not np.any(o["v"][1][:d["water"]]) and np.any(o["v"][1][d["water"]:]), seed
        if b["ragged"]:
            assert 1 in b["counts"] and len(set(b["counts"])) > 1, seed
        assert not (b["weights"] and b["G"]), seed
        structures.add(json.dumps(b["opts"]))
        seen.update(name for name, on in (("dz != dx", para["dz"] != para["dx"]), ("water", d["water"]), ("ragged", b["ragged"]), ("weights", b["weights"]),
                                          ("gauge", b["G"]), ("conditioned twin", b["cond_fname"]),
                                          ("directional", any("das_sensitivity" in sh for k, sh in d["sv"].items() if GA.is_shot(k)))) if on)
    want = {"dz != dx", "water", "ragged", "weights", "gauge", "conditioned twin", "directional"}
    assert want <= seen, sorted(want - seen)
    assert len(structures) >= 4, structures


def test_born_ref_is_the_derivative_of_the_oracle_s_gathers_on_every_draw(oracle, sides):
    worst = 0.0
    for seed in SEEDS:
        o, scale = sides[seed]
        assert o is not None, seed
        b, pb, sv = o["b"], o["d"]["pb"], o["d"]["sv"]
        para = pb["para"]
        if b["G"]:      # the one-cell member channels, which the gauge gathers are a fixed linear map of
            para, sv = {k: val for k, val in para.items() if k != "das_gauge_length"}, GA.member_survey(sv, b["G"], b["vertical"])
        stf, ids = pb["Stf"].numpy(), pb["Shot_ids"].numpy()
        ref = o["raw"]["dsyn"]
        best = {}
        for eps in (1.0, 0.1):
            e = np.float32(eps)
            hi = oracle_gathers(oracle, [a + e * c for a, c in zip(o["m"], o["v"])], stf, ids, para, sv)
            lo = oracle_gathers(oracle, [a - e * c for a, c in zip(o["m"], o["v"])], stf, ids, para, sv)
            for c in COMPS:
                k = ROW[c]
                fd = np.concatenate([((p[k] - q[k]) / (2.0 * eps)).ravel() for p, q in zip(hi, lo)])
                got = np.concatenate([r[k].astype(np.float64).ravel() for r in ref])
                assert fd.shape == got.shape and np.abs(fd).max() > 0, (seed, c)
                best[c] = min(best.get(c, np.inf), C.rel(C.d64(got, fd), fd))
        print("born fuzz seed %2d: born_ref against the finite difference of the oracle's gathers (vx, vz, ett) %s" % (seed, " ".join("%.1e" % best[c] for c in ("vx", "vz", "ett"))))
        worst = max(worst, max(best.values()))
        for c in COMPS:
            assert best[c] <= 1e-2, (seed, c, best[c])
    print("worst %.1e" % worst)
