"""The oracle side of tests/test_gpu_exact_adjoint_fuzz.py on its default 16 seeds, on the CPU: what draw_exact writes is held by a
digest; every draw has a live record at some scale and a target for every comparison (so no default seed reaches the xfail branch on
the GPU); J d is close to the residual (cos >= 0.5), which is what makes <g, d> decide something; between them the draws hold what the
fuzz is for; on the layer draws born_ref is the derivative of the oracle's gathers channel by channel; and the comparison can fail: the
reference's own adjoint misses <W J v, J d> on a layer draw by at least 5 x the tolerance."""
import hashlib
import json

import numpy as np
import pytest

import exact_adjoint_ref as X
import fuzz_common as C
import fuzz_draws as D
from born_ref import COMPS, GRADS, ROW, shifted_gradient
from fuzz_sides import channel_peaks, describe_exact, exact_oracle_side, oracle_gathers

SEEDS = C.DEFAULT_SEEDS
EXACT_DRAWS_DIGEST = "9bb263de52c84a96bc52f061cdadf7ce736d4fe53a17f665ef819449283953c3"


def test_exact_fuzz_draws_are_what_they_were(tmp_path, monkeypatch):
    """What draw_exact adds to the first 16 draws -- layer mode and its cells, the seeds of v, the counts and weights it changes in
    draw_born's dict -- and the two files it rewrites hash to the digest taken when the generator was written.  The weights of a layer draw
    are draw_born's own (fuzz_draws.born_raw): where draw_born uses them they must be the same."""
    for v in C.ENV:
        monkeypatch.delenv(v, raising=False)
    h = hashlib.sha256()
    for seed in SEEDS:
        d = D.draw_problem(tmp_path / ("s%d" % seed), seed, 1)
        b = D.draw_born(d, seed)
        if b["weights"]:
            assert tuple(b["weights"][1:]) == tuple(D.born_raw(seed)[0][k] for k in ("w_vx", "w_vz")), seed
        e = D.draw_exact(d, b, seed)
        h.update(json.dumps(e, sort_keys=True).encode())
        h.update(json.dumps(dict(b, cond_fname=bool(b["cond_fname"])), sort_keys=True).encode())
        h.update(json.dumps({k: v for k, v in d["pb"]["para"].items() if k not in ("survey_fname", "data_dir_name", "scratch_dir_name")}, sort_keys=True).encode())
        h.update(json.dumps(json.load(open(d["pb"]["survey_fname"])), sort_keys=True).encode())
    assert h.hexdigest() == EXACT_DRAWS_DIGEST


@pytest.fixture(scope="module")
def sides(oracle, oracle_nvfma, tmp_path_factory):
    """{seed: (exact_oracle_side's dict or None, scale)} of the default seeds, with the re-draw of the GPU test"""
    return C.default_sides(exact_oracle_side, tmp_path_factory.mktemp("exact_fuzz"), oracle, oracle_nvfma)


def _strip_of(pb, z, x):
    for name, ((z0, z1), (x0, x1)) in D.strips(pb).items():
        if z0 <= z <= z1 and x0 <= x <= x1:
            yield name


def test_exact_fuzz_draws_have_targets_and_cover_what_the_fuzz_is_for(sides):
    count = dict(layer=0, ragged=0, gauge=0, weights=0, water=0, narrow=0, wide=0, edge=0)
    count["directional layer"] = 0
    structures = set()
    for seed in SEEDS:
        o, scale = sides[seed]
        assert o is not None and scale <= 4, "seed %d: the wave does not reach the channels" % seed
        b, d, e, ref = o["b"], o["d"], o["e"], o["ref"]
        pb = d["pb"]
        print("exact fuzz seed %d (%s): build spread %r, cond_g %.1e, cos(W^1/2 J d, W^1/2 r) %.3f, cos(J v, J d) %.3f"
              % (seed, describe_exact(o, scale), {k: "%.1e" % y for k, y in o["yard"].items()}, o["cond_g"], ref["cos_dr"],
                 ref["vw"] / o["cmp"]["<v,JTw>"][2]))
        assert o["target"], (seed, o["yard"], o["cond_g"])
        assert ref["cos_dr"] >= 0.5, (seed, ref["cos_dr"])
        omega = X.mask_omega(pb)
        for pert in (o["v"], o["dm"]):
            assert all(np.abs(a[omega]).max() > 0 and not np.any(a[~omega]) for a in pert), seed
            if d["water"]:
                assert not np.any(pert[1][:d["water"]]), seed
        assert [len(w["ett"]) for w in ref["w"]] == b["counts"], seed
        if e["layer"]:
            assert not b["G"] and b["weights"] and b["weights"][1] > 0 and b["weights"][2] > 0, seed
            nPml, nzc, nx = pb["nPml"], pb["nz_pad"] - pb["nPad"], pb["nx_pad"]
            assert 6 <= len(e["cells"]) <= 12 and max(b["counts"]) == len(e["cells"]), seed
            held = set()
            for z, x in e["cells"]:
                assert 2 <= z <= nzc - 3 and 2 <= x <= nx - 3, (seed, z, x)
                assert z < nPml or x < nPml or x >= nx - nPml, (seed, z, x, "not inside a strip")
                held.update(_strip_of(pb, z, x))
            assert held == {"top", "left", "right"}, (seed, held)
            assert any(x == nx - nPml for _, x in e["cells"]), seed
            if any("das_sensitivity" in sh for k, sh in d["sv"].items() if k.startswith("shot")):
                assert e["cells"][-1][1] == nx - 3, (seed, e["cells"])      # a directional channel on the last column of the update region
                count["directional layer"] += 1
            count["edge"] += any(z == 2 or x == 2 for z, x in e["cells"])      # a channel that reaches row or column 1
            # every channel is alive: its own peak (over the shots that hold it) against the largest, per weighted component
            peaks = channel_peaks(ref["syn"], b)
            for c in COMPS:
                print("    %s peaks / largest: %s" % (c, " ".join("%.1e" % peaks[(c, ch)] for ch in range(len(e["cells"])))))
            assert min(peaks.values()) >= 1e-3, (seed, peaks)
        if b["ragged"]:
            assert 1 in b["counts"] and len(set(b["counts"])) > 1, seed
        structures.add(json.dumps(b["opts"]))
        for name, on in (("layer", e["layer"]), ("ragged", b["ragged"]), ("gauge", b["G"]), ("weights", b["weights"]), ("water", d["water"]),
                         ("narrow", pb["nx_pad"] <= 64), ("wide", pb["nx_pad"] > 64)):
            count[name] += bool(on)
    print(count, len(structures))
    assert count["layer"] >= 3 and count["ragged"] >= 3 and count["gauge"] >= 2 and count["weights"] >= 3 and count["water"] >= 2, count
    assert count["narrow"] >= 1 and count["wide"] >= 1, count
    assert count["edge"] >= 2 and count["directional layer"] >= 1, count      # both ends of the update region (exact_adjoint.hpp: V^T on R only)
    assert len(structures) >= 4, structures


def test_born_ref_is_the_derivative_of_the_oracle_s_gathers_in_the_layers(oracle, sides):
    """born_ref against the central finite difference of oracle.cufd(calc_id 2) on every layer draw, PER CHANNEL and component (method
    and bound 1e-2 of tests/test_born_fuzz_reference.py: rel-L2, best of eps in {1, 0.1})."""
    worst = 0.0
    for seed in SEEDS:
        o, scale = sides[seed]
        if o is None or not o["e"]["layer"]:
            continue
        pb, sv = o["d"]["pb"], o["d"]["sv"]
        para, stf, ids = pb["para"], pb["Stf"].numpy(), pb["Shot_ids"].numpy()
        ref = o["ref"]["raw"]["dsyn"]
        best = {}
        for eps in (1.0, 0.1):
            s = np.float32(eps)
            hi = oracle_gathers(oracle, [a + s * c for a, c in zip(o["m"], o["v"])], stf, ids, para, sv)
            lo = oracle_gathers(oracle, [a - s * c for a, c in zip(o["m"], o["v"])], stf, ids, para, sv)
            for i, (p, q, r) in enumerate(zip(hi, lo, ref)):
                for c in COMPS:
                    k = ROW[c]
                    fd = (p[k] - q[k]) / (2.0 * eps)
                    for ch in range(fd.shape[0]):
                        assert np.abs(fd[ch]).max() > 0, (seed, i, c, ch)
                        best[(i, c, ch)] = min(best.get((i, c, ch), np.inf), C.rel(C.d64(r[k][ch], fd[ch]), fd[ch]))
        print("exact fuzz seed %2d: born_ref against the finite difference of the oracle's gathers, worst channel %.1e, median %.1e"
              % (seed, max(best.values()), float(np.median(list(best.values())))))
        worst = max(worst, max(best.values()))
        bad = {k: val for k, val in best.items() if val > 1e-2}
        assert not bad, (seed, bad)
    assert worst > 0.0, "no layer draw among the default seeds"
    print("worst %.1e" % worst)


def test_the_reference_adjoint_misses_the_cross_product_on_a_layer_draw(oracle, sides):
    """A weaker adjoint must fail: the oracle's gradient at obs = syn - J d (what a re-exported backward pass would give for J^T W J d)
    against <W J v, J d>, on the scale of the GPU test."""
    misses = {}
    for seed in SEEDS:
        o, scale = sides[seed]
        if o is None or not o["e"]["layer"]:
            continue
        pb, sv, b, ref = o["d"]["pb"], o["d"]["sv"], o["b"], o["ref"]
        g = shifted_gradient(oracle, pb, sv, b, o["m"], ref["syn"], ref["jd"])
        r, _, s = o["cmp"]["<v,JTw>"]
        misses[seed] = abs(X.model_dot(o["v"], [g[k] for k in GRADS]) - r) / s
        print("exact fuzz seed %d: the reference's adjoint misses <W J v, J d> by %.2e of |W^1/2 J v| |W^1/2 J d|" % (seed, misses[seed]))
    assert misses and max(misses.values()) >= 5.0 * X.TOL, misses
