"""The reference that the gauge-channel GPU tests rest on (tests/gauge_ref.py, oracle.cufd(adj_src=...)), checked on the CPU: the
adjoint-source hook is the oracle's residual path, a one-cell gauge is the plain oracle, the member-survey gradient is the gradient of
the gauge misfit (finite differences), the refactored fuzz draws are what they were, and every default seed of the gauge fuzz
(tests/test_gpu_gauge_fuzz.py) has a parity target and the 16 between them cover the draw space."""
import hashlib
import json

import numpy as np
import pytest

import fuzz_common as C
import fuzz_draws as D
import gauge_ref as R
import problems as P
from fuzz_sides import gauge_oracle_side


def _problem(tmp_path, **kw):
    opts = dict(nz=50, nx=90, nPml=10, nSteps=260, nshots=2, hetero=True)
    opts.update(kw)
    pb = P.make_problem(str(tmp_path), **opts)
    lam, mu, den = pb["lame_init"]
    pb["lame_init"] = ((lam * 1.05).contiguous(), mu, den)      # residuals of the size of the data
    return pb


def test_adjoint_source_hook_is_the_residual_path(oracle, tmp_path):
    """adj_src = obs - syn with the first sample zeroed (gpuMinus) gives the plain call's gradients and gStf bit for bit; the hook is
    refused together with conditioning keys, for another calc_id and with a wrong shape."""
    pb = _problem(tmp_path, nSteps=150)
    stf, ids = pb["Stf"].numpy(), pb["Shot_ids"].numpy()
    obs = oracle.cufd(*[t.numpy() for t in pb["lame_true"]], stf, 2, ids, pb["para"], pb["survey"])["syn"]
    init = [t.numpy() for t in pb["lame_init"]]
    plain = oracle.cufd(*init, stf, 1, ids, pb["para"], pb["survey"], obs=obs)
    r = obs[:, 3] - plain["syn"][:, 3]
    r[:, :, 0] = 0.0
    for kw in (dict(obs=obs), dict()):
        hook = oracle.cufd(*init, stf, 1, ids, pb["para"], pb["survey"], adj_src=r, **kw)
        assert np.abs(plain["gDen"]).max() > 0 and np.abs(plain["gStf"]).max() > 0
        for k in ("gLambda", "gMu", "gDen", "gStf", "syn"):
            assert np.array_equal(hook[k], plain[k]), k
    assert oracle.cufd(*init, stf, 1, ids, pb["para"], pb["survey"], adj_src=r, obs=obs)["misfit"] == plain["misfit"]
    with pytest.raises(ValueError):
        oracle.cufd(*init, stf, 1, ids, dict(pb["para"], filter=[4.0, 8.0, 35.0, 50.0]), pb["survey"], obs=obs, adj_src=r)
    with pytest.raises(ValueError):
        oracle.cufd(*init, stf, 0, ids, pb["para"], pb["survey"], obs=obs, adj_src=r)
    with pytest.raises(ValueError):
        oracle.cufd(*init, stf, 1, ids, pb["para"], pb["survey"], obs=obs, adj_src=r[:, :-1])


@pytest.mark.parametrize("fiber", ["horizontal", "vertical", "directional"])
def test_gauge_of_one_cell_through_the_reference_is_the_plain_oracle(oracle, tmp_path, fiber):
    """G = 1 through gauge_ref.reference: gathers, gradients and gStf bit for bit those of the plain oracle call (the float64 residual
    of two float32 numbers rounds to the float32 difference); the misfit, a float64 sum here and the reference's float32 tree
    reduction there, to 1e-6."""
    kw = dict(das_fiber="vertical") if fiber == "vertical" else dict(das_sensitivity="random") if fiber == "directional" else {}
    pb = _problem(tmp_path, nSteps=150, **kw)
    stf, ids = pb["Stf"].numpy(), pb["Shot_ids"].numpy()
    obs = oracle.cufd(*[t.numpy() for t in pb["lame_true"]], stf, 2, ids, pb["para"], pb["survey"])["syn"]
    init = [t.numpy() for t in pb["lame_init"]]
    plain = oracle.cufd(*init, stf, 1, ids, pb["para"], pb["survey"], obs=obs)
    ref = R.reference(oracle, init, stf, ids, dict(pb["para"], das_gauge_length=pb["para"]["dx"]), pb["survey"], 1, obs[:, 3])
    assert np.abs(plain["gMu"]).max() > 0
    for k in ("gLambda", "gMu", "gDen", "gStf"):
        assert np.array_equal(ref[k], plain[k]), k
    for i in range(len(ids)):
        assert np.array_equal(ref["gauge"][i].astype(np.float32), plain["syn"][i, 3])
        assert np.array_equal(ref["own"][i], plain["syn"][i, :3])
    assert abs(ref["misfit"] - plain["misfit"]) <= 1e-6 * plain["misfit"]


def test_member_survey_of_ragged_and_directional_vertical_shots():
    """member_survey: channel-major members along the axis, sensitivities repeated per member, per-shot channel counts kept."""
    sv = {"nShots": 2,
          "shot0": dict(z_src=2, x_src=5, nrec=2, z_rec=[7, 9], x_rec=[4, 6], das_sensitivity=[[1, 2, 0, 3, 0, 0], [4, 5, 0, 6, 0, 0]]),
          "shot1": dict(z_src=2, x_src=8, nrec=1, z_rec=[11], x_rec=[3], das_sensitivity=[[7, 8, 0, 9, 0, 0]])}
    m = R.member_survey(sv, 4, True)
    assert m["nShots"] == 2 and m["shot0"]["nrec"] == 10 and m["shot1"]["nrec"] == 5
    assert m["shot0"]["z_rec"] == [5, 6, 7, 8, 9, 7, 8, 9, 10, 11] and m["shot0"]["x_rec"] == [4] * 5 + [6] * 5
    assert m["shot1"]["z_rec"] == [9, 10, 11, 12, 13] and m["shot1"]["x_rec"] == [3] * 5
    assert np.array_equal(np.asarray(m["shot0"]["das_sensitivity"])[:, 0], [1] * 5 + [4] * 5)
    h = R.member_survey(sv, 3, False)
    assert h["shot0"]["x_rec"] == [3, 4, 5, 5, 6, 7] and h["shot0"]["z_rec"] == [7] * 3 + [9] * 3
    ks, w = R.members(6)
    assert ks.tolist() == [-3, -2, -1, 0, 1, 2, 3] and abs(w.sum() - 1.0) < 1e-15 and w[0] == w[-1] == 0.5 / 6


@pytest.mark.parametrize("case", ["horizontal-3", "horizontal-6", "vertical-5", "directional-8"])
def test_gauge_gradient_is_consistent_with_finite_differences(oracle, tmp_path, case):
    """The construction every oracle comparison of gauge channels rests on -- member j of channel c is given w_j times its channel's
    residual -- is the gradient of the gauge misfit  1/2 sum_c (obs_c - sum_j w_j ett_cj)^2:  <g, d> against central finite differences
    of that misfit along the normalised density gradient, as test_oracle_vertical_fibre_gradient_is_consistent_with_finite_differences
    does it and with its bound, 5 % (the reference's adjoint is an approximate transpose).  Heterogeneous models, two shots.
    Measured: 3.1 % (G 3), 2.0 % (G 6), 0.4 % (vertical, G 5), 1.4 % (directional, G 8)."""
    fiber, G = case.rsplit("-", 1)[0], int(case.rsplit("-", 1)[1])
    vertical, directional = fiber == "vertical", fiber == "directional"
    kw = dict(rec_z=30)
    if vertical:
        kw["das_fiber"] = "vertical"
    if directional:
        kw.update(das_sensitivity="random", nrec_stride=2)
    pb = _problem(tmp_path, **kw)
    para, sv = dict(pb["para"]), json.loads(json.dumps(pb["survey"]))
    for k in range(2):      # keep every member inside the physical grid
        sh = sv["shot%d" % k]
        keep = [i for i in range(sh["nrec"]) if 6 <= sh["x_rec"][i] < 90 - 6 and 6 <= sh["z_rec"][i] < 50 - 6]
        assert keep
        sh["z_rec"], sh["x_rec"], sh["nrec"] = [sh["z_rec"][i] for i in keep], [sh["x_rec"][i] for i in keep], len(keep)
        if directional:
            sh["das_sensitivity"] = [sh["das_sensitivity"][i] for i in keep]
    para["das_gauge_length"] = G * (para["dz"] if vertical else para["dx"])
    stf, ids = pb["Stf"].numpy(), pb["Shot_ids"].numpy()
    obs = [a.astype(np.float32) for a in R.forward(oracle, [t.numpy() for t in pb["lame_true"]], stf, ids, para, sv, G)[0]]
    lam, mu, den = [t.numpy() for t in pb["lame_init"]]
    r0 = R.reference(oracle, (lam, mu, den), stf, ids, para, sv, G, obs)
    assert r0["misfit"] > 0 and np.abs(r0["gDen"]).max() > 0

    def misfit(den_):
        tot = 0.0
        for o, g in zip(obs, R.forward(oracle, (lam, mu, den_), stf, ids, para, sv, G)[0]):
            r = o.astype(np.float64) - g
            r[:, 0] = 0.0
            tot += float(np.sum(r * r))
        return 0.5 * tot

    d = r0["gDen"] / np.abs(r0["gDen"]).max()
    eps = 2.0     # kg/m^3
    fd = (misfit(den + eps * d) - misfit(den - eps * d)) / (2 * eps)
    gd = float((r0["gDen"].astype(np.float64) * d).sum())
    print("gauge finite differences, %s: fd %.6e, <g, d> %.6e, deviation %.2e" % (case, fd, gd, abs(fd - gd) / abs(gd)))
    assert abs(fd - gd) <= 0.05 * abs(gd), (case, fd, gd)


FUZZ_DRAWS_DIGEST = "a9dddcb0733c30ac13c0eae4234f8917a34601c66d66ca4a2fac2976e90d8528"


def test_fuzz_draws_are_what_they_were(tmp_path, monkeypatch):
    """What tests/test_gpu_fuzz.py hands to its first oracle call -- the observed model, source function, shots, parameter file, survey of
    fuzz_draws.draw_problem -- and its kernel options, seeds 0 ... 15, hash to the digest taken from that file before its drawing part
    became a function of its own."""
    for v in C.ENV:
        monkeypatch.delenv(v, raising=False)
    h = hashlib.sha256()
    for seed in range(16):
        d = D.draw_problem(tmp_path / ("s%d" % seed), seed, 1)
        pb = d["pb"]
        for a in [t.numpy() for t in D.observed_model(pb)] + [pb["Stf"].numpy(), pb["Shot_ids"].numpy()]:
            h.update(np.ascontiguousarray(a).tobytes())
        h.update(json.dumps({k: v for k, v in pb["para"].items() if k not in ("survey_fname", "data_dir_name", "scratch_dir_name")}, sort_keys=True).encode())
        h.update(json.dumps(d["sv"], sort_keys=True).encode())
        h.update(json.dumps(d["opts"], sort_keys=True).encode())
    assert h.hexdigest() == FUZZ_DRAWS_DIGEST


def test_gauge_fuzz_draws_have_parity_targets(tmp_path, oracle, oracle_nvfma):
    """The default seeds of test_random_problem_matches_oracle_with_gauge, oracle side only: NONE lacks a parity target (signal at the
    channels with the record at scale 1, 2 or 4; the two oracle builds within 1e-2 of each other; conditioning term <= 1e-2), and the
    16 draws between them contain every axis / kind, odd and even G, an overlapping line, a ragged shot list, a bound-touching channel,
    a conditioned draw and a water layer."""
    seen = set()
    for seed, (o, scale) in C.default_sides(gauge_oracle_side, tmp_path, oracle, oracle_nvfma).items():
        assert o is not None, "seed %d: the wave does not reach the channels" % seed
        g = o["g"]
        print("gauge fuzz seed %d: %s G %d %s ragged %r touch %r conditioned %r water %d scale %d noise %.1e cond %.1e"
              % (seed, g["mode"], g["G"], g["set"], g["ragged"], g["touch"], o["conditioned"], o["d"]["water"], scale, o["noise_rel"], o["cond_g"]))
        assert o["target"], (seed, o["noise_rel"], o["cond_g"])
        seen.update([g["mode"], "odd" if g["G"] % 2 else "even", g["set"]])
        seen.update(name for name, on in (("ragged", g["ragged"]), ("touch", g["touch"]), ("conditioned", o["conditioned"]), ("water", o["d"]["water"])) if on)
        if g["ragged"]:
            assert 1 in g["counts"] and len(set(g["counts"])) > 1
    want = set(D.MODES) | {"odd", "even", "overlapping line", "ragged", "touch", "conditioned", "water"}
    assert want <= seen, sorted(want - seen)
