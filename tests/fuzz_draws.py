"""The generators of the fuzz tests: everything a seed draws, and nothing that compares.  Every generator draws every quantity for every
seed, used or not, and later ingredients come from generators of their own, so that the geometry of a seed stays what the other fuzz
files see; tests/test_gauge_reference.py, tests/test_born_fuzz_reference.py and tests/test_exact_adjoint_fuzz_reference.py hold digests of
the first 16 seeds' draws
(draw_problem; draw_gauge, draw_born and draw_exact change its draw for tests/test_gpu_gauge_fuzz.py, test_gpu_born_fuzz.py and
test_gpu_exact_adjoint_fuzz.py, whose docstrings say what they draw; draw_pseudo_hessian adds to it, and changes nothing, for
tests/test_gpu_pseudo_hessian_fuzz.py; draw_conditioned puts draw_born's draw under live conditioning keys for
tests/test_gpu_conditioned_gn_fuzz.py, its digest is in tests/test_conditioned_fuzz_reference.py; draw_envelope writes that draw once
more with if_envelope_misfit for tests/test_gpu_envelope_fuzz.py, its digest is in tests/test_envelope_fuzz_reference.py; draw_robust writes
it once more under robust_misfit / robust_delta / robust_quantile for tests/test_gpu_robust_fuzz.py, its digest is in
tests/test_robust_fuzz_reference.py; draw_w2 writes it once more under if_w2_misfit / w2_beta for tests/test_gpu_w2_fuzz.py, its digest is
in tests/test_w2_fuzz_reference.py)."""
import json
import os

import numpy as np

import born_ref as B
import exact_adjoint_ref as X
from gauge_ref import COND_KEYS

OPTION_SETS = [dict(), dict(batch=0), dict(batch=1, batch_f=2, batch_b=1), dict(batch=1, batch_f=3, batch_b=3), dict(batch_order=0),
               dict(batch=0, fwd_lanes=2), dict(line_fuse=0), dict(bwd_fuse=0), dict(early=3, rho_fly=3), dict(amu_fly=3)]


def draw_problem(tmp_path, seed, scale):
    """Everything a seed draws, the problem written under tmp_path: -> dict(pb, sv, opts, extra, kind, want_cross, water, nSteps, f0).
    The problem of the seed at `scale` times its record length (the re-draw of fuzz_common.settle)."""
    import problems as P
    rng = np.random.default_rng(1000 + seed)
    nPml = int(rng.integers(4, 13))
    nz, nx = int(rng.integers(24, 60)), int(rng.integers(30, 100))
    nPad = int(rng.integers(0, 9))
    nSteps = int(rng.integers(90, 200)) * scale
    nshots = int(rng.integers(1, 5))
    # spacings, time step and peak frequency from a generator of their own (the geometry of a seed is what it was before they
    # varied): 5 ... 25 m cells, dz within 30 % of dx, a Courant number of 0.25 ... 0.8 for the fastest cell, 8 ... 40 Hz
    rq = np.random.default_rng(77000 + seed)
    dx = float(np.round(rq.uniform(5.0, 25.0), 2))
    dz = float(np.round(dx * rq.uniform(0.7, 1.3), 2))
    dt = float(rq.uniform(0.25, 0.8) * min(dz, dx) / (3800.0 * 1.05 * np.sqrt(2.0) * (9.0 / 8.0 + 1.0 / 24.0)))
    f0 = float(np.round(max(rq.uniform(8.0, 40.0), 3.0 / (nSteps * dt)), 1))   # the wavelet's peak (1.2 / f0) inside the first 40 % of the record
    tweak = os.environ.get("SEPFWI_FUZZ_TWEAK", "").split(",")      # diagnosis: the same draw with one ingredient changed
    if "square" in tweak:
        dz = dx
    if "lowf" in tweak:
        f0 = float(np.round(max(8.0, 3.0 / (nSteps * dt)), 1))
    if os.environ.get("SEPFWI_FUZZ_DIAG"):
        print("seed %d: nz %d nx %d nPml %d nPad %d nSteps %d nshots %d dx %.2f dz %.2f dt %.3e f0 %.1f (Courant %.2f, %.1f points per shortest S wavelength)"
              % (seed, nz, nx, nPml, nPad, nSteps, nshots, dx, dz, dt, f0, 3990.0 * dt * 1.65 / min(dx, dz), 1400.0 / (2.5 * f0) / max(dx, dz)))
    pb = P.make_problem(str(tmp_path), nz=nz, nx=nx, nPml=nPml, nSteps=nSteps, nshots=nshots, nPad=nPad, hetero=True, seed=seed,
                        src_z=int(rng.integers(1, 5)), rec_z=int(rng.integers(2, nz - 3)), dh=dx, dz=dz, dt=dt, f0=f0)
    sv = json.load(open(pb["survey_fname"]))
    kind = int(rng.integers(0, 3))
    if kind == 1:      # every 2nd .. 4th cell
        step = int(rng.integers(2, 5))
        for k in range(nshots):
            sh = sv["shot%d" % k]
            sh["x_rec"], sh["z_rec"] = sh["x_rec"][::step], sh["z_rec"][::step]
            sh["nrec"] = len(sh["x_rec"])
    elif kind == 2:    # scattered channels, the same for all shots (the oracle front end wants one nrec)
        m = int(rng.integers(3, 15))
        xs = rng.integers(1, nx - 1, size=m).tolist()
        zs = rng.integers(1, nz - 1, size=m).tolist()
        for k in range(nshots):
            sh = sv["shot%d" % k]
            sh["x_rec"], sh["z_rec"], sh["nrec"] = [int(v) for v in xs], [int(v) for v in zs], m
    json.dump(sv, open(pb["survey_fname"], "w"))
    opts = OPTION_SETS[int(rng.integers(0, len(OPTION_SETS)))]
    if os.environ.get("SEPFWI_FUZZ_OPTS"):      # diagnosis: the same draw with other kernel options ("amu_fly=0,rho_fly=0")
        opts = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in os.environ["SEPFWI_FUZZ_OPTS"].split(",")}
    # extensions, drawn last so that the geometry of a seed does not depend on them: per-channel directional sensitivities
    # (survey key das_sensitivity) and the data-conditioning chain (band-pass, cross-correlation misfit, source-signature update)
    extra = int(rng.integers(0, 6))
    if os.environ.get("SEPFWI_FUZZ_NOEXTRA"):   # diagnosis: the same geometry without the extension it drew
        extra = 0
    if extra == 1:
        for k in range(nshots):
            sh = sv["shot%d" % k]
            sens = np.zeros((sh["nrec"], 6))
            sens[:, [0, 3, 1]] = rng.uniform(-1.0, 1.0, (sh["nrec"], 3))
            sh["das_sensitivity"] = sens.tolist()
        json.dump(sv, open(pb["survey_fname"], "w"))
    want_cross = False
    if extra in (2, 4, 5):
        para = dict(pb["para"])
        if extra != 5:
            para["filter"] = [0.12 * f0, 0.32 * f0, 1.8 * f0, 2.8 * f0]
        if extra == 2:
            want_cross = bool(rng.integers(0, 2))
        elif kind != 2:
            # source-signature update, with (4) and without (5) the band-pass.  Not for scattered channels: their amplitudes span
            # tens of decades, ONE channel dominates the least-squares filter, which then fits it exactly -- the misfit collapses
            # to rounding level and its gradient is noise on both sides (seed 232 of a round-3 sweep: misfit 1.7e-4 of 1.4e4)
            para["if_src_update"] = True
        json.dump(para, open(pb["para_fname"], "w"))
        pb["para"] = para
    # a water layer (mu = 0) over the top rows in one draw of four -- the LAST draw, so that everything above is what it was for a
    # seed before the layer was added (round 3: 1 / mu^2 of a fluid cell met a zero spray weight in the gradient finalisation)
    w = 0
    if int(rng.integers(0, 4)) == 0 and "nowater" not in tweak:
        w = nPml + int(rng.integers(2, max(3, nz // 3)))
        P.add_water(pb, w)
    return dict(pb=pb, sv=sv, opts=opts, extra=extra, kind=kind, want_cross=want_cross, water=w, nSteps=nSteps, f0=f0)


def observed_model(pb):
    """The "observed" model = the true model made 8 % stiffer / 3 % denser everywhere: residuals of the size of the data, so the gradient is
    well conditioned against float32 round-off (with a residual 1e-3 of the data, 1e-7 of forward noise -- e.g. two equally valid FMA
    contractions -- is already 1e-3 of the gradient).  -> three contiguous tensors"""
    lam_t, mu_t, den_t = pb["lame_true"]
    return (lam_t * 1.08).contiguous(), (mu_t * 0.95).contiguous(), (den_t * 1.03).contiguous()


def ragged_counts(rg, n, nshots, ragged):
    """Per-shot channel counts out of n and the shot that keeps a single channel, drawn whether used or not.  -> the counts: ragged ones
    with a single-channel shot and at least two different counts, else n for every shot."""
    counts = [int(c) for c in rg.integers(1, n + 1, size=nshots)]
    single = int(rg.integers(0, nshots))
    if not ragged:
        return [n] * nshots
    counts[single] = 1
    if len(set(counts)) == 1:
        counts[(single + 1) % nshots] = n
    return counts


# ---- gauge channels ------------------------------------------------------------------------------------------------------------
GAUGE_SEED0 = 52000      # offset of the gauge generator's seeds (test_gauge_fuzz_draws_have_parity_targets holds for the default 16)
MODES = ("horizontal", "vertical", "directional-horizontal", "directional-vertical")
SETS = ("overlapping line", "line", "scattered")
SIDES = ("top", "bottom", "left", "right")


def member_bounds(nz, nx, nPml, vertical, directional):
    """Padded cells where check_gauge_members (csrc/das_gauge.cpp) accepts a member: (zlo, zhi, xlo, xhi), inclusive.  nz, nx unpadded."""
    nzc, nxp = nz + 2 * nPml, nx + 2 * nPml
    return (1 if (vertical or directional) else 0, nzc - 1 - (1 if directional else 0),
            0 if (vertical and not directional) else 1, nxp - 1 - (1 if directional else 0))


def draw_gauge(d, seed):
    """Replaces the channels of the draw d (draw_problem) by gauge channels and rewrites its two files.  -> dict(G, mode,
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
    ragged = bool(rg.integers(0, 2)) and nshots > 1
    counts = ragged_counts(rg, n, nshots, ragged)
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
        # no source update for scattered channels, as in draw_problem (one channel dominates the least-squares filter, the misfit
        # collapses to rounding level and its gradient is noise on both sides)
        para.pop("if_src_update", None)
    json.dump(sv, open(pb["survey_fname"], "w"))
    json.dump(para, open(pb["para_fname"], "w"))
    pb["para"] = para
    return dict(G=G, mode=MODES[mode], vertical=vertical, directional=directional, set=SETS[cs], stride=stride, ragged=ragged, counts=counts,
                touch=SIDES[side] if touch else None, bad_survey=bad)


# ---- Born modelling --------------------------------------------------------------------------------------------------------------
BORN_SEED0 = 91000
BORN_OPTION_SETS = [dict(), dict(bz=1), dict(bz=4), dict(xcd_remap=0), dict(rho_fly=0), dict(amu_fly=0), dict(rk_lazy=0), dict(bwd_fuse=0),
                    dict(quiet_skip=1), dict(batch=0)]


def born_raw(seed):
    """What draw_born draws for a seed before it looks at the problem, and its generator, from which the channel counts follow.
    mode 0: joint weights, 1: gauge length, 2 and 3: the draw's own channels and misfit"""
    rg = np.random.default_rng(BORN_SEED0 + seed)
    raw = dict(want_cond=int(rg.integers(0, 4)) == 0, opts=BORN_OPTION_SETS[int(rg.integers(0, len(BORN_OPTION_SETS)))],
               want_ragged=bool(rg.integers(0, 2)), mode=int(rg.integers(0, 4)))
    raw["w_vx"], raw["w_vz"] = [float(np.round(w, 3)) for w in rg.uniform(0.1, 1.0, 2)]
    raw["G"] = int(rg.integers(2, 6))
    raw["vertical"] = bool(rg.integers(0, 2))
    raw["stride"], raw["start"], raw["cross_u"] = int(rg.integers(1, raw["G"] + 2)), int(rg.integers(0, 3)), float(rg.uniform())
    return raw, rg


def draw_born(d, seed):
    """Changes the draw d (draw_problem) as the docstring of tests/test_gpu_born_fuzz.py says and rewrites its two files.  Every quantity is drawn
    for every seed, used or not, so that one ingredient never shifts another.
    -> dict(opts, cond_fname (or None), ragged, counts, weights ((1, w_vx, w_vz) or None), G (0: none), vertical)."""
    pb, sv = d["pb"], d["sv"]
    nPml, nPad = pb["nPml"], pb["nPad"]
    nz, nx = pb["nz_pad"] - 2 * nPml - nPad, pb["nx_pad"] - 2 * nPml
    nshots = int(pb["Shot_ids"].numel())
    raw, rg = born_raw(seed)
    want_cond, opts, mode, w_vx, w_vz, G, vertical = [raw[k] for k in ("want_cond", "opts", "mode", "w_vx", "w_vz", "G", "vertical")]
    stride, start, cross_u = raw["stride"], raw["start"], raw["cross_u"]
    para = {k: v for k, v in pb["para"].items() if k not in COND_KEYS}
    if mode == 1:       # a line of gauge channels along the gauge's axis, every member inside the physical grid
        h = G // 2
        na, nc = (nz, nx) if vertical else (nx, nz)
        along = np.arange(h + 1 + start, na - h - 1, stride)
        cross = np.full(along.size, 2 + int(cross_u * (nc - 4)))
        z, x = (along, cross) if vertical else (cross, along)
        for k in range(nshots):
            sh = sv["shot%d" % k]
            sh["z_rec"], sh["x_rec"], sh["nrec"] = [int(a) for a in z], [int(a) for a in x], int(along.size)
            sh.pop("das_sensitivity", None)
        para.pop("das_fiber", None)
        if vertical:
            para["das_fiber"] = "vertical"
        para["das_gauge_length"] = G * float(para["dz"] if vertical else para["dx"])
    else:
        G, vertical = 0, para.get("das_fiber", "horizontal") == "vertical"
    weights = None
    if mode == 0:
        weights = (1.0, w_vx, w_vz)
        para.update(misfit_w_ett=1.0, misfit_w_vx=w_vx, misfit_w_vz=w_vz)
    n = int(sv["shot0"]["nrec"])
    ragged = raw["want_ragged"] and nshots > 1 and n > 1
    counts = ragged_counts(rg, n, nshots, ragged)
    if ragged:
        for k in range(nshots):
            sh = sv["shot%d" % k]
            sh["z_rec"], sh["x_rec"], sh["nrec"] = sh["z_rec"][:counts[k]], sh["x_rec"][:counts[k]], counts[k]
            if "das_sensitivity" in sh:
                sh["das_sensitivity"] = sh["das_sensitivity"][:counts[k]]
    json.dump(sv, open(pb["survey_fname"], "w"))
    json.dump(para, open(pb["para_fname"], "w"))
    pb["para"] = para
    cond_fname = None
    if want_cond:       # the same problem with a live conditioning key, a session of its own (plain misfit: a joint one refuses the key)
        cond_fname = os.path.join(os.path.dirname(pb["para_fname"]), "para_cond.json")
        cdir = os.path.join(os.path.dirname(pb["para_fname"]), "Cond_Data")
        os.makedirs(cdir, exist_ok=True)
        json.dump(dict({k: val for k, val in para.items() if not k.startswith("misfit_w_")}, if_cross_misfit=True, data_dir_name=cdir), open(cond_fname, "w"))
    return dict(opts=opts, cond_fname=cond_fname, ragged=ragged, counts=counts, weights=weights, G=G, vertical=vertical)


# ---- the exact adjoint -------------------------------------------------------------------------------------------------------------
EXACT_SEED0 = 95400
MAX_LAYER_CHANNELS = 12


def strips(pb):
    """{name: (rows lo..hi, columns lo..hi)} of the three strips of layer mode, padded cells, inclusive"""
    nPml, nzc, nx = pb["nPml"], pb["nz_pad"] - pb["nPad"], pb["nx_pad"]
    half = max(nPml, nzc // 2)
    return dict(top=((2, nPml - 1), (2, nx - 3)), left=((2, half), (2, nPml - 1)), right=((2, half), (nx - nPml, nx - 3)))


def draw_exact(d, b, seed):
    """Changes the draw (d: draw_problem, b: draw_born) as the docstring of tests/test_gpu_exact_adjoint_fuzz.py says, rewrites its two files and updates b (counts,
    ragged, weights).  -> dict(layer, cells (padded (z, x) of the layer channels, else None), v_seeds)."""
    pb, sv = d["pb"], d["sv"]
    nPml = pb["nPml"]
    nshots = int(pb["Shot_ids"].numel())
    rg = np.random.default_rng(EXACT_SEED0 + seed)
    layer = int(rg.integers(0, 3)) == 0 and not b["G"]
    m = int(rg.integers(6, MAX_LAYER_CHANNELS + 1))
    place = [0, 1, 2] + [int(p) for p in rg.integers(0, 3, size=MAX_LAYER_CHANNELS - 3)]
    u = rg.uniform(size=(MAX_LAYER_CHANNELS, 2))
    sens = rg.uniform(-1.0, 1.0, (MAX_LAYER_CHANNELS, 3))
    cu = rg.uniform(size=4)
    single = int(rg.integers(0, 4)) % nshots
    v_seeds = [int(s) for s in rg.integers(0, 2 ** 31, size=2)]
    cells = None
    if layer:
        st = strips(pb)
        cells = []
        directional = "das_sensitivity" in sv["shot0"]
        if directional:     # the last channel on the LAST column of the update region: a directional channel reaches column x+1 outside it
            place[m - 1] = 2
        for k in range(m):
            (z0, z1), (x0, x1) = st[("top", "left", "right")[place[k]]]
            z, x = z0 + int(u[k, 0] * (z1 - z0 + 1)), x0 + int(u[k, 1] * (x1 - x0 + 1))
            if k == 2:
                x = pb["nx_pad"] - nPml      # the column inside the x strip of S and outside that of V
            if directional and k == m - 1:
                x = pb["nx_pad"] - 3
            cells.append((min(z, z1), min(x, x1)))
        counts = [min(m, 1 + int(c * m)) for c in cu[:nshots]]
        if b["ragged"]:     # (draw_born: more than one shot) a single-channel shot and one with the whole list
            counts[single], counts[(single + 1) % nshots] = 1, m
        else:
            counts = [m] * nshots
        for k in range(nshots):
            sh = sv["shot%d" % k]
            directional = "das_sensitivity" in sh
            n = counts[k]
            sh["z_rec"], sh["x_rec"], sh["nrec"] = [int(z - nPml) for z, _ in cells[:n]], [int(x - nPml) for _, x in cells[:n]], n
            if directional:
                full = np.zeros((n, 6))
                full[:, [0, 3, 1]] = sens[:n]
                sh["das_sensitivity"] = full.tolist()
        w_vx, w_vz = [born_raw(seed)[0][k] for k in ("w_vx", "w_vz")]
        para = dict(pb["para"], misfit_w_ett=1.0, misfit_w_vx=w_vx, misfit_w_vz=w_vz)
        b.update(counts=counts, weights=(1.0, w_vx, w_vz))
        json.dump(sv, open(pb["survey_fname"], "w"))
        json.dump(para, open(pb["para_fname"], "w"))
        pb["para"] = para
    return dict(layer=layer, cells=cells, v_seeds=v_seeds)


def perturbations(d, e):
    """v and d of that docstring -> two lists of three float32 (nz_pad, nx_pad) arrays"""
    pb, w = d["pb"], d["water"]
    v = [B.f32(a + c) for a, c in zip(X.smooth_v(pb, e["v_seeds"][0], w), X.white_v(pb, e["v_seeds"][1], w))]
    dm = [t.numpy() - i.numpy() for t, i in zip(pb["lame_true"], pb["lame_init"])]
    dm[1][:int(w)] = 0.0
    return v, X.on_omega(pb, dm)


# ---- conditioned Gauss-Newton (if_win / filter) ------------------------------------------------------------------------------------
COND_SEED0 = 98035      # offset of the generator (how it was chosen: tests/test_conditioned_fuzz_reference.py)
COND_MODES = ("filter", "window", "both", "narrow")      # the names of cond_gn_ref
COND_CORNERS = (0.1, 0.5, 0.6, 1.2)      # x f0.  Not cond_gn_ref.CORNERS: on these draws that band leaves |C C d| within 7 % of |C d|
COND_MAX = (4, 128)                      # shots and channels a draw_problem survey can hold: the window draws have this shape for every seed


def conditioned_raw(seed):
    """What draw_conditioned draws for a seed before it looks at the problem or at a gather; every quantity for every seed."""
    rg = np.random.default_rng(COND_SEED0 + seed)
    raw = dict(mode=COND_MODES[int(rg.integers(0, len(COND_MODES)))], u1=rg.uniform(size=COND_MAX), u2=rg.uniform(size=COND_MAX),
               weights=rg.uniform(0.5, 2.0, COND_MAX), want_empty=int(rg.integers(0, 4)) == 0, empty_u=[float(u) for u in rg.uniform(size=2)])
    raw["v_seeds"] = [int(s) for s in rg.integers(0, 2 ** 31, size=2)]
    return raw


def energy_times(trace, dt, T):
    """(t10, t90): the times at which the cumulative energy of a trace reaches 10 % and 90 %; (0, T) for a dead trace"""
    e = np.cumsum(np.asarray(trace, np.float64) ** 2)
    if not e[-1] > 0:
        return 0.0, T
    return float(np.searchsorted(e, 0.1 * e[-1]) * dt), float(np.searchsorted(e, 0.9 * e[-1]) * dt)


def draw_conditioned(d, b, seed, syn):
    """The draw (d: draw_problem, b: draw_born) under live conditioning keys, as the docstring of tests/test_gpu_conditioned_gn_fuzz.py
    says.  syn: per shot the REFERENCE's (nrec, nSteps) axial-strain gather at lame_init (plain oracle build) -- the windows are placed on
    its arrivals, from the reference side alone.  No joint weights: misfit_w_* leave d's parameter file and b["weights"] becomes None
    (config.cpp refuses them together with conditioning keys); everything else of draw_born stays, and d's two files remain the same
    problem WITHOUT the keys.  The conditioned pair is written next to them with cond_gn_ref.write_files.
    -> dict(mode, pb (a shallow copy of d["pb"] on the conditioned pair, with "survey" and "data_dir"), empty ((shot, channel) of the
    empty window, or None), v_seeds)."""
    import cond_gn_ref as G
    pb, sv = d["pb"], d["sv"]
    raw = conditioned_raw(seed)
    mode = raw["mode"]
    plain = {k: v for k, v in pb["para"].items() if k not in COND_KEYS and not k.startswith("misfit_w_")}
    json.dump(plain, open(pb["para_fname"], "w"))
    pb["para"] = plain
    b["weights"] = None
    ids = [int(i) for i in pb["Shot_ids"].tolist()]
    dt, f0 = float(plain["dt"]), float(plain["f0"])
    T = int(plain["nSteps"]) * dt
    empty = None
    if raw["want_empty"]:
        k = int(raw["empty_u"][0] * len(ids))
        empty = (k, int(raw["empty_u"][1] * int(sv["shot%d" % ids[k]]["nrec"])))
    csv = dict(sv)
    for k, sid in enumerate(ids):
        sh = dict(sv["shot%d" % sid])
        n = int(sh["nrec"])
        assert np.shape(syn[k]) == (n, int(plain["nSteps"])) and n <= COND_MAX[1] and k < COND_MAX[0], (seed, k, np.shape(syn[k]))
        t = [energy_times(syn[k][r], dt, T) for r in range(n)]
        sh["win_start"] = [float(t10 + raw["u1"][k, r] * 0.5 * (t90 - t10)) for r, (t10, t90) in enumerate(t)]
        sh["win_end"] = [float(t90 + raw["u2"][k, r] * 0.5 * (T - t90)) for r, (t10, t90) in enumerate(t)]
        sh["weights"] = [float(w) for w in raw["weights"][k, :n]]
        sh["src_weight"] = 0.3 + 0.05 * k      # below 1: with 3.0 the window's gain and the filter's loss cancel in mode "both"
        if empty is not None and empty[0] == k:
            sh["win_end"][empty[1]] = sh["win_start"][empty[1]]      # "Window error 1": the trace passes untouched
        csv["shot%d" % sid] = sh
    para = dict(plain)
    if mode in ("filter", "both"):
        para["filter"] = [c * f0 for c in COND_CORNERS]
    if mode == "narrow":
        para["filter"] = G.narrow(f0)
    if mode in ("window", "both"):
        para["if_win"] = True
    cpb = dict(pb)
    cpb["para_fname"], cpb["para"] = G.write_files(pb, "cond", para, csv)
    cpb["survey"], cpb["survey_fname"], cpb["data_dir"] = csv, cpb["para"]["survey_fname"], cpb["para"]["data_dir_name"]
    return dict(mode=mode, pb=cpb, empty=empty, v_seeds=raw["v_seeds"])


# ---- the envelope misfit (if_envelope_misfit) on the conditioned draw ----------------------------------------------------------------
ENV_SEED0 = 99001      # offset of the generator (how it was chosen: tests/test_envelope_fuzz_reference.py)
ENV_KEY = "if_envelope_misfit"


def envelope_raw(seed):
    """What draw_envelope draws for a seed, every quantity for every seed: whether the key stands alone (one draw in four) and the seed
    of the white-noise gathers a test may want."""
    rg = np.random.default_rng(ENV_SEED0 + seed)
    return dict(alone=int(rg.integers(0, 4)) == 0, noise_seed=int(rg.integers(0, 2 ** 31)))


def draw_envelope(d, c, seed):
    """The conditioned draw (d: draw_problem, c: draw_conditioned) written a second time with if_envelope_misfit added: the pair
    "env" next to the conditioned pair, same survey (windows, weights, src_weight), same keys plus the key -- or, in one draw of four,
    the key ALONE: if_win and filter leave the file (nobody then reads the survey's windows) and C is the plain end taper.  The pair
    "env_twin" is the same file without the key, for the bit-identity checks.  draw_conditioned's own pair stays what it is.
    -> dict(mode (c's, or "alone"), alone, pb, twin (shallow copies of c["pb"] on the two pairs), noise_seed)."""
    import cond_gn_ref as G
    raw = envelope_raw(seed)
    cpb = c["pb"]
    para = {k: v for k, v in cpb["para"].items() if k not in ("survey_fname", "data_dir_name")}
    if raw["alone"]:
        para = {k: v for k, v in para.items() if k not in COND_KEYS}
    out = {}
    for name, extra in (("pb", {ENV_KEY: True}), ("twin", {})):
        pb = dict(cpb)
        pb["para_fname"], pb["para"] = G.write_files(d["pb"], "env" if name == "pb" else "env_twin", dict(para, **extra), cpb["survey"])
        pb["survey_fname"], pb["data_dir"] = pb["para"]["survey_fname"], pb["para"]["data_dir_name"]
        out[name] = pb
    return dict(mode="alone" if raw["alone"] else c["mode"], alone=raw["alone"], noise_seed=raw["noise_seed"], **out)


# ---- the diagonal pseudo-Hessian ---------------------------------------------------------------------------------------------------
PH_SEED0 = 97255     # (of the offsets 97000 ... 97399 the one whose default 16 seeds hold the most of the 17 option sets: 13, with batch = 0 and batch = 1 on multi-shot draws)
PH_EVERY = (1, 2, 3, 5)
PH_OPTION_SETS = OPTION_SETS + [o for o in BORN_OPTION_SETS if o not in OPTION_SETS]      # the union, every structure once


def draw_pseudo_hessian(d, seed):
    """What tests/test_gpu_pseudo_hessian_fuzz.py adds to the draw d (draw_problem), from a generator of its own; d and its two files
    stay what they are -- conditioning keys, directional channels and water layer included, none of which the result may depend on.
    -> dict(every, entry ("backward": a gradient call, "forward": a misfit-only call with pseudo_hessian=), opts, fetch ("ops": the
    operator's return value, "capi": sepfwi_pseudo_hessian_arm / sepfwi_get_pseudo_hessian into host memory))."""
    rg = np.random.default_rng(PH_SEED0 + seed)
    every = PH_EVERY[int(rg.integers(0, len(PH_EVERY)))]
    entry = ("backward", "forward")[int(rg.integers(0, 2))]
    opts = PH_OPTION_SETS[int(rg.integers(0, len(PH_OPTION_SETS)))]
    fetch = ("ops", "capi")[int(rg.integers(0, 2))]
    return dict(every=every, entry=entry, opts=opts, fetch=fetch)


# ---- the robust misfits (robust_misfit / robust_delta / robust_quantile) on the conditioned draw ------------------------------------
ROB_SEED0 = 99411      # offset of the generator (how it was chosen: tests/test_robust_fuzz_reference.py)
ROB_KINDS = ("huber", "cauchy")
ROB_DELTAS = (0.1, 0.5)
ROB_QUANTILES = (None, 0.99, 1.0)      # None: the key is absent from the file, the library's default 0.9
ROB_STEPS = (0.9, 0.99, 1.0)           # where a quantile steps to when more than half of the call's traces are dead (draw_robust)
ROB_KEYS = ("robust_misfit", "robust_delta", "robust_quantile")


def robust_raw(seed):
    """What draw_robust draws for a seed, every quantity for every seed: whether the keys stand alone (one draw in four), the penalty,
    robust_delta, robust_quantile (None: absent from the file) and the seed of the spikes."""
    rg = np.random.default_rng(ROB_SEED0 + seed)
    return dict(alone=int(rg.integers(0, 4)) == 0, kind=ROB_KINDS[int(rg.integers(0, len(ROB_KINDS)))],
                delta=ROB_DELTAS[int(rg.integers(0, len(ROB_DELTAS)))], quantile=ROB_QUANTILES[int(rg.integers(0, len(ROB_QUANTILES)))],
                spike_seed=int(rg.integers(0, 2 ** 31)))


def draw_robust(d, c, seed, steps=0):
    """The conditioned draw (d: draw_problem, c: draw_conditioned) written a second time under the robust keys: the pair "rob" next to
    the conditioned pair, same survey (windows, weights, src_weight), same keys plus robust_misfit, robust_delta and (unless the draw
    left it to the default) robust_quantile -- or, in one draw of four, the keys ALONE: if_win and filter leave the file and C is the
    plain end taper.  The pair "rob_twin" is the same file without the three keys, for the bit-identity checks.  draw_conditioned's own
    pair stays what it is.  steps: how often the quantile has stepped up along ROB_STEPS (fuzz_sides.robust_oracle_side decides that
    on the reference side, where more than half of the call's traces are dead); a stepped quantile is written into the file.
    -> dict(mode (c's, or "alone"), alone, kind, delta, quantile (the value in force), drawn (the value drawn, None: default),
    stepped, pb, twin (shallow copies of c["pb"] on the two pairs), spike_seed)."""
    import cond_gn_ref as G
    raw = robust_raw(seed)
    cpb = c["pb"]
    para = {k: v for k, v in cpb["para"].items() if k not in ("survey_fname", "data_dir_name")}
    if raw["alone"]:
        para = {k: v for k, v in para.items() if k not in COND_KEYS}
    q0 = 0.9 if raw["quantile"] is None else raw["quantile"]
    q = ROB_STEPS[min(ROB_STEPS.index(q0) + steps, len(ROB_STEPS) - 1)]
    keys = {"robust_misfit": raw["kind"], "robust_delta": raw["delta"]}
    if raw["quantile"] is not None or q != q0:
        keys["robust_quantile"] = q
    out = {}
    for name, extra in (("pb", keys), ("twin", {})):
        pb = dict(cpb)
        pb["para_fname"], pb["para"] = G.write_files(d["pb"], "rob" if name == "pb" else "rob_twin", dict(para, **extra), cpb["survey"])
        pb["survey_fname"], pb["data_dir"] = pb["para"]["survey_fname"], pb["para"]["data_dir_name"]
        out[name] = pb
    return dict(mode="alone" if raw["alone"] else c["mode"], alone=raw["alone"], kind=raw["kind"], delta=raw["delta"], quantile=q,
                drawn=raw["quantile"], stepped=q != q0, spike_seed=raw["spike_seed"], **out)


# ---- the W2 misfit (if_w2_misfit / w2_beta) on the conditioned draw -------------------------------------------------------------------
W2_SEED0 = 99826      # offset of the generator (how it was chosen: tests/test_w2_fuzz_reference.py)
W2_BETAS = (None, 0.5, 8.0, 16.0)      # None: the key is absent from the file, the library's default 3.0
W2_KEYS = ("if_w2_misfit", "w2_beta")


def w2_raw(seed):
    """What draw_w2 draws for a seed, every quantity for every seed: whether the key stands alone (one draw in four), w2_beta (None:
    absent from the file), and whether one OBSERVED channel of the one-shot call's shot is silenced (one draw in two; dead_u: which)."""
    rg = np.random.default_rng(W2_SEED0 + seed)
    return dict(alone=int(rg.integers(0, 4)) == 0, beta=W2_BETAS[int(rg.integers(0, len(W2_BETAS)))], dead=bool(rg.integers(0, 2)),
                dead_u=float(rg.uniform()))


def draw_w2(d, c, seed):
    """The conditioned draw (d: draw_problem, c: draw_conditioned) written a second time under if_w2_misfit: the pair "w2" next to the
    conditioned pair, same survey (windows, weights, src_weight), same keys plus the key and (unless the draw left it to the default)
    w2_beta -- or, in one draw of four, the key ALONE: if_win and filter leave the file and C is the plain end taper.  The pair
    "w2_twin" is the same file without the two keys, for the bit-identity checks.  draw_conditioned's own pair stays what it is.
    The files hold nothing of the silenced channel: it is a property of the observed DATA (exact zeros in one channel: a dead trace,
    A == 0, beside live ones), applied by fuzz_sides.w2_oracle_side where the shot holds two channels or more.
    -> dict(mode (c's, or "alone"), alone, beta (the value in force), drawn (the value drawn, None: default), dead, dead_u, pb, twin
    (shallow copies of c["pb"] on the two pairs))."""
    import cond_gn_ref as G
    raw = w2_raw(seed)
    cpb = c["pb"]
    para = {k: v for k, v in cpb["para"].items() if k not in ("survey_fname", "data_dir_name")}
    if raw["alone"]:
        para = {k: v for k, v in para.items() if k not in COND_KEYS}
    keys = {"if_w2_misfit": True}
    if raw["beta"] is not None:
        keys["w2_beta"] = raw["beta"]
    out = {}
    for name, extra in (("pb", keys), ("twin", {})):
        pb = dict(cpb)
        pb["para_fname"], pb["para"] = G.write_files(d["pb"], "w2" if name == "pb" else "w2_twin", dict(para, **extra), cpb["survey"])
        pb["survey_fname"], pb["data_dir"] = pb["para"]["survey_fname"], pb["para"]["data_dir_name"]
        out[name] = pb
    return dict(mode="alone" if raw["alone"] else c["mode"], alone=raw["alone"], beta=3.0 if raw["beta"] is None else raw["beta"],
                drawn=raw["beta"], dead=raw["dead"], dead_u=raw["dead_u"], **out)
