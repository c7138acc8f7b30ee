"""The reference for the diagonal pseudo-Hessian (csrc/pseudo_hessian.hpp, sepfwi_pseudo_hessian_arm), shared by every test that
compares it with the CPU oracle.

The reference package has nothing of the kind, so this is an unpinned extension: its reference is the DEFINITION evaluated in float64
numpy on the oracle's float32 fields.  The oracle's stencil kernels and helpers are exported, so this module is the oracle's forward
shot loop (ofwi_shot, oracle/torchfwi_oracle.c) restated as a Python step loop over them (tests/oracle_loop.py) exactly as
geophone_ref._shot does it, with the accumulation between the source add and velocity(1): at that point vz, vx still stand as at the start of the step and szz, sxx, sxz carry this step's update and source.
It returns the loop's gathers too: they equal oracle.cufd(..., calc_id 2) bit for bit (tests/test_pseudo_hessian_reference.py), which
makes it the oracle's loop.

Definition (interior nPml <= z <= nzc - 1 - nPml, nPml <= x <= nx - 1 - nPml; forward steps it = 0 ... nSteps - 2 with
it % every == 0, weight every; D-/D+ the 4th-order staggered stencils):
    a = D-z vz, b = D-x vx, s = D+z vx + D+x vz;   Fz = D+z szz + D-x sxz, Fx = D-z sxz + D+x sxx
    E_lam += every (a + b)^2,  E_mu += every (4 a^2 + 4 b^2 + s^2),  E_rho += every ((ba^2/2 Fz)^2 + (bb^2/2 Fx)^2)
    H_lam = 2 (1e6 dt)^2 E_lam,  H_mu = (1e6 dt)^2 E_mu,  H_rho = dt^2 E_rho,    summed over the shots, zero outside the interior.
Either oracle build serves (oracle_loop: the loop only calls the build's exported kernels); the nvfma build gives a second valid rounding
of the same fields, the yardstick of tests/test_gpu_pseudo_hessian_fuzz.py.  The five combinations are exported (combinations), and
tests/test_pseudo_hessian_fuzz_reference.py holds them against the oracle's own stress and velocity kernels on dz != dx."""
import numpy as np

import oracle_loop as OL

C1, C2 = 9.0 / 8.0, 1.0 / 24.0

# The two small problems of the tests (problems.make_problem): 2 and 3 row segments of 64 columns per interior row, the last one ragged.
PROBLEM_A = dict(nz=50, nx=90, nPml=10, nSteps=260, nshots=2, hetero=True, rec_z=30)
PROBLEM_B = dict(nz=40, nx=150, nSteps=400, nshots=3)


NAMES = ("hLambda", "hMu", "hDen")
FLOOR = 1e-30      # a cell is LIVE where the un-scaled accumulator E = H / constant reaches this: six decades above the smallest normal float32
#                    (1.2e-38) that the GPU's float32 sets and outputs hold, so a live cell's sum is carried by normal numbers


def masks(pb):
    """(interior, ring) of a problem (problems.make_problem), bool (nz_pad, nx_pad): the cells the definition covers, and the outermost of
    them -- the first and last interior row and column"""
    nPml, nzc, nx = pb["nPml"], pb["nz_pad"] - pb["nPad"], pb["nx_pad"]
    inside = np.zeros((pb["nz_pad"], nx), bool)
    inside[nPml:nzc - nPml, nPml:nx - nPml] = True
    core = np.zeros_like(inside)
    core[nPml + 1:nzc - nPml - 1, nPml + 1:nx - nPml - 1] = True
    return inside, inside & ~core


def live_cells(H, dt):
    """per array of H = (hLambda, hMu, hDen): the cells whose E = H / constant is at least FLOOR"""
    return [np.asarray(h, np.float64) >= FLOOR * c for h, c in zip(H, constants(dt))]


def live_shares(H, pb):
    """(share of the interior, share of the ring) that is live, the smallest of the three arrays"""
    inside, ring = masks(pb)
    live = live_cells(H, pb["para"]["dt"])
    return min(float(l[inside].mean()) for l in live), min(float(l[ring].mean()) for l in live)


# The directed edge cases of tests/test_gpu_pseudo_hessian_fuzz.py: dz = 0.8 dx, shots in opposite corners of the physical grid (and one in
# its middle) so that all four edges of the interior are lit; nSteps the smallest multiple of 10 at which the whole ring is live.
# name: (make_problem's grid, shots, nSteps, kernel options).  xmax = nx + nPml - 1: the last 64-column segment holds 64, 1, 64, 1 interior
# columns; rows x segments = 23, 46, 46, 69 waves, never a multiple of the 4 waves of a block.
EDGE_CASES = {
    "xmax 63": (dict(nz=23, nx=60, nPml=4, nPad=3), 3, 30, dict()),
    "xmax 64, lanes": (dict(nz=23, nx=61, nPml=4, nPad=3), 3, 40, dict(batch=0)),
    "xmax 127, three shots in one sub-batch": (dict(nz=23, nx=124, nPml=4, nPad=3), 3, 70, dict(batch=1, batch_split=1)),
    "xmax 128, a lane used twice": (dict(nz=23, nx=125, nPml=4, nPad=3), 3, 70, dict(batch=0, fwd_lanes=2)),
    "nPml 2": (dict(nz=20, nx=30, nPml=2, nPad=2), 2, 30, dict()),
    "nPml 64, nPad 0": (dict(nz=8, nx=8, nPml=64, nPad=0), 2, 10, dict(batch=0)),
    "nPml 64, nPad 5": (dict(nz=8, nx=8, nPml=64, nPad=5), 2, 10, dict(batch=1)),
}


def edge_problem(workdir, name, nSteps=None):
    """The problem of one of EDGE_CASES, written under workdir.  -> (problem, kernel options)"""
    import json
    import problems as P
    grid, nshots, steps, opts = EDGE_CASES[name]
    nz, nx = grid["nz"], grid["nx"]
    pb = P.make_problem(str(workdir), nSteps=nSteps or steps, nshots=nshots, dh=10.0, dz=8.0, hetero=True, seed=21, rec_x=list(range(1, nx - 1)), rec_z=nz // 2, **grid)
    src = [(1, 1), (nz - 2, nx - 2), (nz // 2, nx // 2)][:nshots]
    sv = pb["survey"]
    for k, (z, x) in enumerate(src):
        sv["shot%d" % k]["z_src"], sv["shot%d" % k]["x_src"] = z, x
    json.dump(sv, open(pb["survey_fname"], "w"))
    return pb, opts


def _shift(f, dx, dz, xs, zs):
    """f[x + dx, z + dz] on the interior block (arrays are [x][z])."""
    return f[xs.start + dx:xs.stop + dx, zs.start + dz:zs.stop + dz]


def _dminus(f, axis, xs, zs, h):   # (c1 (f0 - fm1) - c2 (fp1 - fm2)) / h
    s = (lambda k: _shift(f, k, 0, xs, zs)) if axis == "x" else (lambda k: _shift(f, 0, k, xs, zs))
    return (C1 * (s(0) - s(-1)) - C2 * (s(1) - s(-2))) / h


def _dplus(f, axis, xs, zs, h):    # (c1 (fp1 - f0) - c2 (fp2 - fm1)) / h
    s = (lambda k: _shift(f, k, 0, xs, zs)) if axis == "x" else (lambda k: _shift(f, 0, k, xs, zs))
    return (C1 * (s(1) - s(0)) - C2 * (s(2) - s(-1))) / h


def combinations(f, xs, zs, dz, dx):
    """The five combinations of the definition on the interior block (xs, zs: slices of the [x][z] arrays) of the field set f (a dict
    that holds vz, vx, szz, sxx, sxz), evaluated in float64.  -> (a, b, s, Fz, Fx)"""
    vz, vx, szz, sxx, sxz = [np.asarray(f[k], np.float64) for k in OL.FIELDS]
    a, b = _dminus(vz, "z", xs, zs, dz), _dminus(vx, "x", xs, zs, dx)
    sh = _dplus(vx, "z", xs, zs, dz) + _dplus(vz, "x", xs, zs, dx)
    Fz = _dplus(szz, "z", xs, zs, dz) + _dminus(sxz, "x", xs, zs, dx)
    Fx = _dminus(sxz, "z", xs, zs, dz) + _dplus(sxx, "x", xs, zs, dx)
    return a, b, sh, Fz, Fx


def constants(dt):
    """(c_lam, c_mu, c_rho) with H = c E, from the float32 time step as the session takes it"""
    dtd = float(np.float32(dt))
    return 2.0 * (1e6 * dtd) ** 2, (1e6 * dtd) ** 2, dtd ** 2


def _shot(s, stf, z_src, x_src, z_rec, x_rec, sens, everies, E):
    """Forward loop of one shot of the call s (oracle_loop.Setup); adds into E[every] = [E_lam, E_mu, E_rho] (float64, interior block
    [x][z]).  -> syn (4, nrec, nSteps)."""
    nx, nzc, nPml, dz, dx = s.nx, s.nzc, s.nPml, s.dz, s.dx
    f = s.new_fields()
    xs, zs = slice(nPml, nx - nPml), slice(nPml, nzc - nPml)
    wa = (s.bA[xs, zs].astype(np.float64) ** 2) / 2.0
    wb = (s.bB[xs, zs].astype(np.float64) ** 2) / 2.0
    syn = np.zeros((4, z_rec.size, s.nSteps), np.float32)
    for it in range(s.nSteps - 1):
        acc = [e for e in everies if it % e == 0]
        if acc:    # the velocities as they stand at the start of the step (stress(1) does not change them)
            a, b, sh, _, _ = combinations(f, xs, zs, dz, dx)
            t_lam, t_mu = (a + b) ** 2, 4.0 * a ** 2 + 4.0 * b ** 2 + sh ** 2
        s.stress(f, s.fLam, s.fMu, s.aMu)
        s.add_source(f, stf[it], z_src, x_src)
        if acc:    # the stresses after this step's update and source add
            _, _, _, Fz, Fx = combinations(f, xs, zs, dz, dx)
            t_rho = (wa * Fz) ** 2 + (wb * Fx) ** 2
            for e in acc:
                E[e][0] += e * t_lam
                E[e][1] += e * t_mu
                E[e][2] += e * t_rho
        s.velocity(f, s.bA, s.bB)
        s.record(syn, it + 1, f, z_rec, x_rec, sens)
    return syn


def pseudo_hessian(oracle, Lambda, Mu, Den, Stf, shot_ids, para, survey, every=(1,), per_shot=False):
    """oracle.cufd's arguments (straight fibres or directional channels: only the gathers depend on them).
    -> {every: (hLambda, hMu, hDen)} float64 (nz, nx), summed over shot_ids (per_shot: a list with one such triple per shot), and
    the gathers of the loop: (nshots, 4, nrec, nSteps), or a list of (4, nrec, nSteps) where the shots differ in nrec."""
    s = OL.Setup(oracle, Lambda, Mu, Den, para)
    everies = tuple(int(e) for e in every)
    nz, nx, nzc, nPml, dt = s.nz, s.nx, s.nzc, s.nPml, s.dt
    consts = constants(dt)
    shape = (nx - 2 * nPml, nzc - 2 * nPml)

    def dense(E):
        out = []
        for k in range(3):
            h = np.zeros((nz, nx), np.float64)
            h[nPml:nzc - nPml, nPml:nx - nPml] = (consts[k] * E[k]).T
            out.append(h)
        return tuple(out)

    syn_all, shots = [], []
    total = {e: [np.zeros(shape, np.float64) for _ in range(3)] for e in everies}
    for sid, stf_s, z_src, x_src, z_rec, x_rec, _, sens in s.shots(Stf, shot_ids, survey):
        E = {e: [np.zeros(shape, np.float64) for _ in range(3)] for e in everies}
        syn_all.append(_shot(s, stf_s, z_src, x_src, z_rec, x_rec, sens, everies, E))
        for e in everies:
            for k in range(3):
                total[e][k] += E[e][k]
        if per_shot:
            shots.append({e: dense(E[e]) for e in everies})
    out = {e: dense(total[e]) for e in everies}
    syn = np.stack(syn_all) if len({a.shape for a in syn_all}) == 1 else syn_all
    return (out, syn, shots) if per_shot else (out, syn)
