"""Seeded random small problems WITH DAS gauge channels (parameter key "das_gauge_length"): HIP propagator vs CPU oracle (-m gpu).

Every seed is a draw of tests/test_gpu_fuzz.py (draw_problem: grid, layers, padding, spacings, time step, frequency, shots, kernel
options, band-pass / cross-correlation misfit / source update, water layer) whose channels are then replaced, from a generator of
their own, by gauge channels: G in 2 ... 9; a horizontal, vertical, directional-on-a-horizontal-axis or directional-on-a-vertical-axis
gauge; a line whose neighbouring gauges overlap (stride < G), one whose gauges do not (stride >= G), or scattered channels with a
repeat and a neighbour one cell apart; in half of the multi-shot draws a different channel count per shot, one shot with a single
channel; in one draw of four channel 0 pushed out until its outermost member sits on the last cell the survey check accepts (inside
the absorbing layer: survey coordinates are unpadded, the parser adds nPml) -- and one cell further must be refused.

The reference is tests/gauge_ref.py on both oracle builds; yardsticks and tolerances are those of tests/test_gpu_fuzz.py, none new.
The oracle side of a draw (oracle_side) needs no GPU: tests/test_gauge_reference.py runs it on the default seeds and asserts that
every one of them has a parity target, so the xfail branch below is never what the default seeds report."""
import json
import os

import numpy as np
import pytest

import gauge_ref as R
import problems as P
import test_gpu_fuzz as F

pytestmark = pytest.mark.gpu

GAUGE_SEED0 = 52000      # offset of the gauge generator's seeds (test_gauge_fuzz_draws_have_parity_targets holds for the default 16)
MODES = ("horizontal", "vertical", "directional-horizontal", "directional-vertical")
SETS = ("overlapping line", "line", "scattered")
SIDES = ("top", "bottom", "left", "right")

_SEEDS = ([int(v) for v in os.environ["SEPFWI_GAUGE_FUZZ_SEEDS"].split(",")] if os.environ.get("SEPFWI_GAUGE_FUZZ_SEEDS")
          else list(range(int(os.environ.get("SEPFWI_GAUGE_FUZZ_N", "16")))))


def member_bounds(nz, nx, nPml, vertical, directional):
    """Padded cells where check_gauge_members (csrc/das_gauge.cpp) accepts a member: (zlo, zhi, xlo, xhi), inclusive.  nz, nx unpadded."""
    nzc, nxp = nz + 2 * nPml, nx + 2 * nPml
    return (1 if (vertical or directional) else 0, nzc - 1 - (1 if directional else 0),
            0 if (vertical and not directional) else 1, nxp - 1 - (1 if directional else 0))


def draw_gauge(d, seed):
    """Replaces the channels of the draw d (test_gpu_fuzz.draw_problem) by gauge channels and rewrites its two files.  -> dict(G, mode,
    vertical, directional, set, stride, ragged, touch (side name or None), bad_survey (channel 0 one cell beyond the bound, or None))."""
    pb = d["pb"]
    nPml, nPad = pb["nPml"], pb["nPad"]
    nz, nx = pb["nz_pad"] - 2 * nPml - nPad, pb["nx_pad"] - 2 * nPml
    nshots = int(pb["Shot_ids"].numel())
    rg = np.random.default_rng(GAUGE_SEED0 + seed)
    G = int(rg.integers(2, 10))
    mode = int(rg.integers(0, 4))
    vertical, directional = mode in (1, 3), mode in (2, 3)
    h = G // 2                                        # reach of the outermost member, odd and even G
    na, nc = (nz, nx) if vertical else (nx, nz)       # extent along / across the gauge axis
    cs = int(rg.integers(0, 3))
    stride = 0
    if cs < 2:
        stride = int(rg.integers(1, G)) if cs == 0 else G + int(rg.integers(0, 3))
        cross = int(rg.integers(2, nc - 2))
        along = np.arange(h + 1 + int(rg.integers(0, 3)), na - h - 1, stride)
        cr = np.full(along.size, cross)
    else:
        m = int(rg.integers(4, 15))
        along = rg.integers(h + 1, na - h - 1, size=m)
        cr = rg.integers(2, nc - 2, size=m)
        along[2], cr[2] = along[1], cr[1]                                                        # a repeat
        along[3], cr[3] = (along[1] + 1 if along[1] + 1 < na - h - 1 else along[1] - 1), cr[1]   # a neighbour one cell along the axis
    n = int(along.size)
    assert n >= 2, (seed, n)
    z, x = (along, cr) if vertical else (cr, along)
    z, x = [int(v) for v in z], [int(v) for v in x]
    sens = np.zeros((n, 6))
    sens[:, [0, 3, 1]] = rg.uniform(-1.0, 1.0, (n, 3))
    want_ragged, counts = bool(rg.integers(0, 2)), [int(v) for v in rg.integers(1, n + 1, size=nshots)]
    single = int(rg.integers(0, nshots))
    ragged = want_ragged and nshots > 1
    if ragged:
        counts[single] = 1
        if len(set(counts)) == 1:
            counts[(single + 1) % nshots] = n
    else:
        counts = [n] * nshots
    touch, side = int(rg.integers(0, 4)) == 0, int(rg.integers(0, 4))
    bad = None
    if touch:       # channel 0 (in every shot's list): its outermost member on the last accepted cell of one side
        zlo, zhi, xlo, xhi = member_bounds(nz, nx, nPml, vertical, directional)
        hz, hx = (h, 0) if vertical else (0, h)
        bz, bx = z[0], x[0]
        if side == 0:
            z[0] = zlo + hz - nPml; bz = z[0] - 1
        elif side == 1:
            z[0] = zhi - hz - nPml; bz = z[0] + 1
        elif side == 2:
            x[0] = xlo + hx - nPml; bx = x[0] - 1
        else:
            x[0] = xhi - hx - nPml; bx = x[0] + 1
    sv = d["sv"]

    def put(sv_, z_, x_):
        for k in range(nshots):
            sh = sv_["shot%d" % k]
            sh["z_rec"], sh["x_rec"], sh["nrec"] = z_[:counts[k]], x_[:counts[k]], counts[k]
            sh.pop("das_sensitivity", None)
            if directional:
                sh["das_sensitivity"] = sens[:counts[k]].tolist()

    put(sv, z, x)
    if touch:
        bad = json.loads(json.dumps(sv))
        put(bad, [bz] + z[1:], [bx] + x[1:])
    para = dict(pb["para"])
    para.pop("das_fiber", None)
    if vertical:
        para["das_fiber"] = "vertical"
    para["das_gauge_length"] = G * float(para["dz"] if vertical else para["dx"])
    if cs == 2:
        # no source update for scattered channels, as in test_gpu_fuzz.py (one channel dominates the least-squares filter, the misfit
        # collapses to rounding level and its gradient is noise on both sides)
        para.pop("if_src_update", None)
    json.dump(sv, open(pb["survey_fname"], "w"))
    json.dump(para, open(pb["para_fname"], "w"))
    pb["para"] = para
    return dict(G=G, mode=MODES[mode], vertical=vertical, directional=directional, set=SETS[cs], stride=stride, ragged=ragged, counts=counts,
                touch=SIDES[side] if touch else None, bad_survey=bad)


def _l2(a):
    return float(np.linalg.norm(np.asarray(a, np.float64)))


def oracle_side(tmp_path, oracle, oracle_nvfma, seed, scale):
    """The draw and everything the two oracle builds say about it (no GPU).  -> None when the record ends before the wave reaches the
    channels (the caller draws again with a longer record), else a dict; ["target"] is False where the draw has no parity target."""
    d = F.draw_problem(tmp_path, seed, scale)
    g = draw_gauge(d, seed)
    pb, sv, G = d["pb"], d["sv"], g["G"]
    # "observed" model as in test_gpu_fuzz.py: 8 % stiffer / 3 % denser everywhere, residuals of the size of the data
    lam_t, mu_t, den_t = pb["lame_true"]
    true = ((lam_t * 1.08).contiguous(), (mu_t * 0.95).contiguous(), (den_t * 1.03).contiguous())
    ids = pb["Shot_ids"].numpy()
    stf = pb["Stf"].numpy()
    gauge_t, own_t = R.forward(oracle, [t.numpy() for t in true], stf, ids, pb["para"], sv, G)
    src_scale = float(np.abs(stf).max()) * 1500.0 ** 2 * float(pb["para"]["dt"])
    peak = max(float(np.abs(a).max()) for a in gauge_t)
    if os.environ.get("SEPFWI_FUZZ_DIAG"):
        print("seed %d scale %d: %r; max |ett| / src_scale = %.3e, extra %d, water %d, opts %r, para %r"
              % (seed, scale, {k: v for k, v in g.items() if k != "bad_survey"}, peak / src_scale, d["extra"], d["water"], d["opts"],
                 {k: v for k, v in pb["para"].items() if "fname" not in k and "dir" not in k}))
    if peak < 3e-10 * src_scale:      # only the stencil's numerical precursor (test_gpu_fuzz.py)
        return None
    energy = np.concatenate([(a ** 2).sum(-1) for a in gauge_t])
    if d["want_cross"] and float(energy.min()) > 1e-4 and float(energy.min()) > 1e-6 * float(energy.max()):
        para = dict(pb["para"])
        para["if_cross_misfit"] = True
        json.dump(para, open(pb["para_fname"], "w"))
        pb["para"] = para
    gauge_alt, own_alt = R.forward(oracle_nvfma, [t.numpy() for t in true], stf, ids, pb["para"], sv, G)
    obs = [a.astype(np.float32) for a in gauge_t]
    init = [t.numpy() for t in pb["lame_init"]]
    ref = R.reference(oracle, init, stf, ids, pb["para"], sv, G, obs)
    alt = R.reference(oracle_nvfma, init, stf, ids, pb["para"], sv, G, obs)
    # conditioning of the draw and the cap of the yardstick: the comment at the assertions of test_gpu_fuzz.py
    E_obs = 0.5 * sum(_l2(a) ** 2 for a in obs)
    eps = 2.0 ** -24
    cond_m = 8.0 * eps * float(np.sqrt(abs(ref["misfit"]) * E_obs))
    cond_g = 4.0 * eps * float(np.sqrt(E_obs / max(abs(ref["misfit"]), 1e-300)))
    noise_rel = max(_l2(alt[n] - ref[n]) / max(_l2(ref[n]), 1e-300) for n in ("gLambda", "gMu", "gDen"))
    return dict(d=d, g=g, true=true, obs=obs, gauge_t=gauge_t, own_t=own_t, gauge_alt=gauge_alt, own_alt=own_alt, ref=ref, alt=alt,
                src_scale=src_scale, cond_m=cond_m, cond_g=cond_g, noise_rel=noise_rel, target=(noise_rel <= 1e-2 and cond_g <= 1e-2),
                conditioned=any(k in pb["para"] for k in R.COND_KEYS))


@pytest.mark.parametrize("seed", _SEEDS)   # one-off sweeps: SEPFWI_GAUGE_FUZZ_N=200 (CPU-oracle bound)
def test_random_problem_matches_oracle_with_gauge(tmp_path, oracle, oracle_nvfma, hip_ops, seed):
    """As test_random_problem_matches_oracle: a draw whose record ends before the wave reaches the channels is drawn again with the
    record two, then four times as long."""
    for scale in (1, 2, 4):
        if _attempt(tmp_path / ("x%d" % scale), oracle, oracle_nvfma, hip_ops, seed, scale):
            return
    pytest.xfail("seed %d: the wave does not reach the channels even with a record four times as long" % seed)


def _attempt(tmp_path, oracle, oracle_nvfma, hip_ops, seed, scale):
    from sepfwi import _native, fwi_ops
    from sepfwi import utils as ft
    o = oracle_side(tmp_path, oracle, oracle_nvfma, seed, scale)
    if o is None:
        return False
    d, g, ref, alt = o["d"], o["g"], o["ref"], o["alt"]
    pb, opts, w, nSteps = d["pb"], d["opts"], d["water"], d["nSteps"]
    tag = (seed, g["mode"], g["G"], g["set"], g["touch"], opts)
    d64 = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)))
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
                worse("fwd " + c, d64(got, a) / max(_l2(a), 1e-300))
                assert d64(got, a) <= 1e-4 * _l2(a) + 3.0 * d64(b, a), (tag, c, sid, d64(got, a) / max(_l2(a), 1e-300))
                if c == "ett" and g["touch"]:
                    # the channel in the absorbing layer is weak beside the others: its own trace against its own norm, whenever it
                    # carries more than the precursor level; where every tap lies on cells that are never updated, exactly zero
                    if not np.any(a[0]):
                        assert not np.any(got[0]), (tag, sid, "the bound-touching channel must record exactly zero")
                    elif float(np.abs(a[0]).max()) >= 3e-10 * o["src_scale"]:
                        worse("fwd ett, bound-touching channel", d64(got[0], a[0]) / _l2(a[0]))
                        assert d64(got[0], a[0]) <= 1e-4 * _l2(a[0]) + 3.0 * d64(b[0], a[0]), (tag, sid, "bound-touching channel", d64(got[0], a[0]) / _l2(a[0]))
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
        assert abs(float(m) - ref["misfit"]) <= 1e-4 * abs(ref["misfit"]) + 3.0 * abs(ref["misfit"] - alt["misfit"]) + cond_m + 1e-30, (tag, dev)
        for name, gg, r in (("gLambda", gL, ref["gLambda"]), ("gMu", gM, ref["gMu"]), ("gDen", gD, ref["gDen"])):
            err, noise = _l2(gg.numpy() - r), _l2(alt[name] - r)
            dev[name] = (err / max(_l2(r), 1e-300), noise / max(_l2(r), 1e-300))
            assert err <= (1e-3 + cond_g) * _l2(r) + 3.0 * noise, (tag, name, dev[name], cond_g)
            if w:   # below a water layer the image is held on its own (against the larger of its own norm and 3 % of the whole image's)
                yard = max(_l2(r[w:]), 3e-2 * _l2(r))
                assert _l2(gg.numpy()[w:] - r[w:]) <= (1e-3 + cond_g) * yard + 3.0 * _l2(alt[name][w:] - r[w:]), (tag, name, "below the water")
        nS_ = ref["gStf"].shape[0]
        dev["gStf"] = (_l2(gS.numpy()[:nS_] - ref["gStf"]) / max(_l2(ref["gStf"]), 1e-300), _l2(alt["gStf"] - ref["gStf"]) / max(_l2(ref["gStf"]), 1e-300))
        print("gauge fuzz seed %d (%s, G %d, %s%s%s%s%s, scale %d): %r"
              % (seed, g["mode"], g["G"], g["set"], ", ragged" if g["ragged"] else "", ", touching " + g["touch"] if g["touch"] else "",
                 ", conditioned" if o["conditioned"] else "", ", water" if w else "", scale, dev))
        assert _l2(gS.numpy()[:nS_] - ref["gStf"]) <= (5e-3 + cond_g) * _l2(ref["gStf"]) + 3.0 * _l2(alt["gStf"] - ref["gStf"]), (tag, "gStf", dev)
    return True
