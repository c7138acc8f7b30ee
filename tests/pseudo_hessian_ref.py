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
Default oracle build only (nothing fused)."""
import numpy as np

import oracle_loop as OL

C1, C2 = 9.0 / 8.0, 1.0 / 24.0

# The two small problems of the tests (problems.make_problem): 2 and 3 row segments of 64 columns per interior row, the last one ragged.
PROBLEM_A = dict(nz=50, nx=90, nPml=10, nSteps=260, nshots=2, hetero=True, rec_z=30)
PROBLEM_B = dict(nz=40, nx=150, nSteps=400, nshots=3)


def _shift(f, dx, dz, xs, zs):
    """f[x + dx, z + dz] on the interior block (arrays are [x][z])."""
    return f[xs.start + dx:xs.stop + dx, zs.start + dz:zs.stop + dz]


def _dminus(f, axis, xs, zs, h):   # (c1 (f0 - fm1) - c2 (fp1 - fm2)) / h
    s = (lambda k: _shift(f, k, 0, xs, zs)) if axis == "x" else (lambda k: _shift(f, 0, k, xs, zs))
    return (C1 * (s(0) - s(-1)) - C2 * (s(1) - s(-2))) / h


def _dplus(f, axis, xs, zs, h):    # (c1 (fp1 - f0) - c2 (fp2 - fm1)) / h
    s = (lambda k: _shift(f, k, 0, xs, zs)) if axis == "x" else (lambda k: _shift(f, 0, k, xs, zs))
    return (C1 * (s(1) - s(0)) - C2 * (s(2) - s(-1))) / h


def _shot(s, stf, z_src, x_src, z_rec, x_rec, everies, E):
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
            vz, vx = f["vz"].astype(np.float64), f["vx"].astype(np.float64)
            a, b = _dminus(vz, "z", xs, zs, dz), _dminus(vx, "x", xs, zs, dx)
            sh = _dplus(vx, "z", xs, zs, dz) + _dplus(vz, "x", xs, zs, dx)
            t_lam, t_mu = (a + b) ** 2, 4.0 * a ** 2 + 4.0 * b ** 2 + sh ** 2
        s.stress(f, s.fLam, s.fMu, s.aMu)
        s.add_source(f, stf[it], z_src, x_src)
        if acc:    # the stresses after this step's update and source add
            szz, sxx, sxz = [f[k].astype(np.float64) for k in ("szz", "sxx", "sxz")]
            Fz = _dplus(szz, "z", xs, zs, dz) + _dminus(sxz, "x", xs, zs, dx)
            Fx = _dminus(sxz, "z", xs, zs, dz) + _dplus(sxx, "x", xs, zs, dx)
            t_rho = (wa * Fz) ** 2 + (wb * Fx) ** 2
            for e in acc:
                E[e][0] += e * t_lam
                E[e][1] += e * t_mu
                E[e][2] += e * t_rho
        s.velocity(f, s.bA, s.bB)
        s.record(syn, it + 1, f, z_rec, x_rec, None)
    return syn


def pseudo_hessian(oracle, Lambda, Mu, Den, Stf, shot_ids, para, survey, every=(1,), per_shot=False):
    """oracle.cufd's arguments (straight horizontal or vertical fibres, no directional channels).
    -> {every: (hLambda, hMu, hDen)} float64 (nz, nx), summed over shot_ids (per_shot: a list with one such triple per shot), and
    the gathers (nshots, 4, nrec, nSteps) of the loop."""
    assert oracle.VARIANT == "", "pseudo_hessian_ref restates the unfused oracle build"
    s = OL.Setup(oracle, Lambda, Mu, Den, para)
    everies = tuple(int(e) for e in every)
    nz, nx, nzc, nPml, dt = s.nz, s.nx, s.nzc, s.nPml, s.dt
    dtd = float(np.float32(dt))
    consts = (2.0 * (1e6 * dtd) ** 2, (1e6 * dtd) ** 2, dtd ** 2)
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
        assert sens is None
        E = {e: [np.zeros(shape, np.float64) for _ in range(3)] for e in everies}
        syn_all.append(_shot(s, stf_s, z_src, x_src, z_rec, x_rec, everies, E))
        for e in everies:
            for k in range(3):
                total[e][k] += E[e][k]
        if per_shot:
            shots.append({e: dense(E[e]) for e in everies})
    out = {e: dense(total[e]) for e in everies}
    return (out, np.stack(syn_all), shots) if per_shot else (out, np.stack(syn_all))
