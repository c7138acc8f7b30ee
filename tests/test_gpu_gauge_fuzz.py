"""Seeded random small problems WITH DAS gauge channels (parameter key "das_gauge_length"): HIP propagator vs CPU oracle (-m gpu).

Every seed is a draw of tests/test_gpu_fuzz.py (fuzz_draws.draw_problem: grid, layers, padding, spacings, time step, frequency, shots,
kernel options, band-pass / cross-correlation misfit / source update, water layer) whose channels are then replaced, from a generator of
their own (fuzz_draws.draw_gauge), by gauge channels: G in 2 ... 9; a horizontal, vertical, directional-on-a-horizontal-axis or
directional-on-a-vertical-axis gauge; a line whose neighbouring gauges overlap (stride < G), one whose gauges do not (stride >= G), or
scattered channels with a repeat and a neighbour one cell apart; in half of the multi-shot draws a different channel count per shot, one
shot with a single channel; in one draw of four channel 0 pushed out until its outermost member sits on the last cell the survey check
accepts (inside the absorbing layer: survey coordinates are unpadded, the parser adds nPml) -- and one cell further must be refused.

The reference is tests/gauge_ref.py on both oracle builds (fuzz_sides.gauge_oracle_side, no GPU); yardsticks and tolerances are those of
tests/test_gpu_fuzz.py (tests/fuzz_common.py), none new."""
import json
import os

import numpy as np
import pytest

import fuzz_common as C
import problems as P
from fuzz_common import d64, d_own, l2, rel
from fuzz_sides import gauge_oracle_side

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", C.seeds("SEPFWI_GAUGE_FUZZ"))
def test_random_problem_matches_oracle_with_gauge(tmp_path, oracle, oracle_nvfma, hip_ops, seed):
    """As test_random_problem_matches_oracle, with its re-draw of a record that ends before the wave reaches the channels."""
    from sepfwi import _native, fwi_ops
    from sepfwi import utils as ft
    o, scale = C.settled(gauge_oracle_side, tmp_path, oracle, oracle_nvfma, seed)
    d, g, ref, alt = o["d"], o["g"], o["ref"], o["alt"]
    pb, opts, w, nSteps = d["pb"], d["opts"], d["water"], d["nSteps"]
    tag = (seed, g["mode"], g["G"], g["set"], g["touch"], opts)
    dev = {}

    def worse(key, v):
        dev[key] = max(dev.get(key, 0.0), v)

    with P.kernel_options(**opts):
        if g["touch"]:      # one cell beyond the last accepted one: refused by the survey check, before anything runs
            bad_sv = os.path.join(os.path.dirname(pb["survey_fname"]), "beyond_survey.json")
            bad_para = os.path.join(os.path.dirname(pb["para_fname"]), "beyond.json")
            json.dump(g["bad_survey"], open(bad_sv, "w"))
            json.dump(dict(pb["para"], survey_fname=bad_sv), open(bad_para, "w"))
            with pytest.raises(_native.SepFwiError) as e:
                hip_ops.obscalc(*o["true"], pb["Stf"], 1, pb["Shot_ids"], bad_para)
            assert e.value.code == -1 and "receiver 0 of shot 0" in str(e.value), (tag, str(e.value))
        hip_ops.obscalc(*o["true"], pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
        ids = pb["Shot_ids"].tolist()
        for i, sid in enumerate(ids):
            want = {"ett": (o["gauge_t"][i], o["gauge_alt"][i])}
            for k, c in enumerate(("pr", "vx", "vz")):      # sampled at the channel's own cell: the member survey's centre member
                want[c] = (o["own_t"][i][k], o["own_alt"][i][k])
            for c, (a, b) in want.items():
                got = ft.read_shot_gather(pb["data_dir"], c, sid, nSteps)
                assert got.shape == a.shape, (tag, c, sid, got.shape, a.shape)
                worse("fwd " + c, rel(d64(got, a), a))
                assert C.array_held(got, a, b, C.GATHER_TOL), (tag, c, sid, rel(d64(got, a), a))
                if c == "ett" and g["touch"]:
                    # the channel in the absorbing layer is weak beside the others: its own trace against its own norm, whenever it
                    # carries more than the precursor level; where every tap lies on cells that are never updated, exactly zero
                    if not np.any(a[0]):
                        assert not np.any(got[0]), (tag, sid, "the bound-touching channel must record exactly zero")
                    elif not C.is_precursor(float(np.abs(a[0]).max()), o["src_scale"]):
                        worse("fwd ett, bound-touching channel", d64(got[0], a[0]) / l2(a[0]))
                        assert C.array_held(got[0], a[0], b[0], C.GATHER_TOL), (tag, sid, "bound-touching channel", d64(got[0], a[0]) / l2(a[0]))
        os.makedirs(pb["data_dir"], exist_ok=True)
        for i, sid in enumerate(ids):
            o["obs"][i].tofile(os.path.join(pb["data_dir"], "Shot_ett%d.bin" % sid))
            for k, c in enumerate(("pr", "vx", "vz")):
                np.ascontiguousarray(o["own_t"][i][k]).tofile(os.path.join(pb["data_dir"], "Shot_%s%d.bin" % (c, sid)))
        fwi_ops.release()   # observed data were rewritten behind the session's cache with identical mtimes possible
        lam, mu, den = pb["lame_init"]
        m, gL, gM, gD, gS = hip_ops.backward(lam, mu, den, pb["Stf"], 1, pb["Shot_ids"], pb["para_fname"])
        cond_m, cond_g = o["cond_m"], o["cond_g"]
        if os.environ.get("SEPFWI_FUZZ_DIAG"):
            print("seed %d: misfit HIP %.9e, oracle %.9e, nvcc-FMA oracle %.9e; noise %.2e cond_g %.2e" % (seed, float(m), ref["misfit"], alt["misfit"], o["noise_rel"], cond_g))
        if not o["target"]:
            pytest.xfail("seed %d: no parity target -- the reference algorithm differs from itself by %.1e of the gradient on this draw "
                         "(conditioning term %.1e)" % (seed, o["noise_rel"], cond_g))
        dev["misfit"] = abs(float(m) - ref["misfit"]) / max(abs(ref["misfit"]), 1e-300)
        assert C.scalar_held(float(m), ref["misfit"], alt["misfit"], C.MISFIT_TOL, floor=cond_m + 1e-30), (tag, dev)
        for name, gg in (("gLambda", gL), ("gMu", gM), ("gDen", gD)):
            r = ref[name]
            dev[name] = (rel(d_own(gg.numpy(), r), r), rel(d_own(alt[name], r), r))
            miss = C.gradient_miss(gg.numpy(), r, alt[name], C.GRAD_TOL, cond_g, w, d_own)
            assert not miss, (tag, name, miss, dev[name], cond_g)
        nS_ = ref["gStf"].shape[0]
        dev["gStf"] = (rel(d_own(gS.numpy()[:nS_], ref["gStf"]), ref["gStf"]), rel(d_own(alt["gStf"], ref["gStf"]), ref["gStf"]))
        print("gauge fuzz seed %d (%s, G %d, %s%s%s%s%s, scale %d): %r"
              % (seed, g["mode"], g["G"], g["set"], ", ragged" if g["ragged"] else "", ", touching " + g["touch"] if g["touch"] else "",
                 ", conditioned" if o["conditioned"] else "", ", water" if w else "", scale, dev))
        assert C.array_held(gS.numpy()[:nS_], ref["gStf"], alt["gStf"], C.STF_TOL, cond_g, d_own), (tag, "gStf", dev)
