"""The reference for the diagonal pseudo-Hessian (csrc/pseudo_hessian.hpp, sepfwi_pseudo_hessian_arm), shared by every test that
compares it with the CPU oracle.

The reference package has nothing of the kind, so this is an unpinned extension: its reference is the DEFINITION evaluated in float64
numpy on the oracle's float32 fields.  The oracle's stencil kernels and helpers are exported, so this module is the oracle's forward
shot loop (ofwi_shot, oracle/torchfwi_oracle.c) restated as a Python step loop over ofwi_el_stress / ofwi_el_velocity /
ofwi_model_average / ofwi_cpml_init exactly as geophone_ref._shot does it, with the accumulation between the source add and
velocity(1): at that point vz, vx still stand as at the start of the step and szz, sxx, sxz carry this step's update and source.
It returns the loop's gathers too: they equal oracle.cufd(..., calc_id 2) bit for bit (tests/test_pseudo_hessian_reference.py), which
makes it the oracle's loop.

Definition (interior nPml <= z <= nzc - 1 - nPml, nPml <= x <= nx - 1 - nPml; forward steps it = 0 ... nSteps - 2 with
it % every == 0, weight every; D-/D+ the 4th-order staggered stencils):
    a = D-z vz, b = D-x vx, s = D+z vx + D+x vz;   Fz = D+z szz + D-x sxz, Fx = D-z sxz + D+x sxx
    E_lam += every (a + b)^2,  E_mu += every (4 a^2 + 4 b^2 + s^2),  E_rho += every ((ba^2/2 Fz)^2 + (bb^2/2 Fx)^2)
    H_lam = 2 (1e6 dt)^2 E_lam,  H_mu = (1e6 dt)^2 E_mu,  H_rho = dt^2 E_rho,    summed over the shots, zero outside the interior.
Default oracle build only (nothing fused)."""
import ctypes as C

import numpy as np

from geophone_ref import _Cpml, _fp

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


def _shot(L, prm, media, cz, cx, stf, z_src, x_src, z_rec, x_rec, everies, E):
    """Forward loop of one shot; adds into E[every] = [E_lam, E_mu, E_rho] (float64, interior block [x][z]).  -> syn (4, nrec, nSteps)."""
    nz, nx, nSteps, nPml, nPad, dz, dx, dt, fiber = prm
    fLam, fMu, aMu, bA, bB = media
    nzc = nz - nPad
    c = _Cpml(*([_fp(cz[k * nzc:(k + 1) * nzc]) for k in range(6)] + [_fp(cx[k * nx:(k + 1) * nx]) for k in range(6)]))
    dims = (C.c_int(nz), C.c_int(nx), C.c_float(dt), C.c_float(dz), C.c_float(dx), C.c_int(nPml), C.c_int(nPad))
    f = {k: np.zeros((nx, nz), np.float32) for k in ("vz", "vx", "szz", "sxx", "sxz", "dvz_dz", "dvz_dx", "dvx_dz", "dvx_dx",
                                                     "dszz_dz", "dsxx_dx", "dsxz_dz", "dsxz_dx")}
    p = {k: _fp(v) for k, v in f.items()}
    xs, zs = slice(nPml, nx - nPml), slice(nPml, nzc - nPml)
    wa = (bA[xs, zs].astype(np.float64) ** 2) / 2.0
    wb = (bB[xs, zs].astype(np.float64) ** 2) / 2.0
    syn = np.zeros((4, z_rec.size, nSteps), np.float32)
    src_scale, dtf = np.float32(1500.0 ** 2), np.float32(dt)
    for it in range(nSteps - 1):
        acc = [e for e in everies if it % e == 0]
        if acc:    # the velocities as they stand at the start of the step (stress(1) does not change them)
            vz, vx = f["vz"].astype(np.float64), f["vx"].astype(np.float64)
            a, b = _dminus(vz, "z", xs, zs, dz), _dminus(vx, "x", xs, zs, dx)
            s = _dplus(vx, "z", xs, zs, dz) + _dplus(vz, "x", xs, zs, dx)
            t_lam, t_mu = (a + b) ** 2, 4.0 * a ** 2 + 4.0 * b ** 2 + s ** 2
        L.ofwi_el_stress(p["vz"], p["vx"], p["szz"], p["sxx"], p["sxz"], p["dvz_dz"], p["dvz_dx"], p["dvx_dz"], p["dvx_dx"],
                         _fp(fLam), _fp(fMu), _fp(aMu), C.byref(c), *dims, C.c_int(1), *((None,) * 5))
        amp = np.float32(np.float32(src_scale * stf[it]) * dtf)       # add_source, utilities.cu:524-552
        f["szz"][x_src, z_src] = amp + f["szz"][x_src, z_src]
        f["sxx"][x_src, z_src] = amp + f["sxx"][x_src, z_src]
        if acc:    # the stresses after this step's update and source add
            szz, sxx, sxz = [f[k].astype(np.float64) for k in ("szz", "sxx", "sxz")]
            Fz = _dplus(szz, "z", xs, zs, dz) + _dminus(sxz, "x", xs, zs, dx)
            Fx = _dminus(sxz, "z", xs, zs, dz) + _dplus(sxx, "x", xs, zs, dx)
            t_rho = (wa * Fz) ** 2 + (wb * Fx) ** 2
            for e in acc:
                E[e][0] += e * t_lam
                E[e][1] += e * t_mu
                E[e][2] += e * t_rho
        L.ofwi_el_velocity(p["vz"], p["vx"], p["szz"], p["sxx"], p["sxz"], p["dszz_dz"], p["dsxz_dx"], p["dsxz_dz"], p["dsxx_dx"],
                           _fp(bA), _fp(bB), C.byref(c), *dims, C.c_int(1), *((None,) * 3))
        vx, vz = f["vx"], f["vz"]
        syn[0, :, it + 1] = f["szz"][x_rec, z_rec] + f["sxx"][x_rec, z_rec]
        syn[1, :, it + 1] = vx[x_rec, z_rec]
        syn[2, :, it + 1] = vz[x_rec, z_rec]
        syn[3, :, it + 1] = (vz[x_rec, z_rec] - vz[x_rec, z_rec - 1]) if fiber else (vx[x_rec, z_rec] - vx[x_rec - 1, z_rec])
    return syn


def pseudo_hessian(oracle, Lambda, Mu, Den, Stf, shot_ids, para, survey, every=(1,), per_shot=False):
    """oracle.cufd's arguments (straight horizontal or vertical fibres, no directional channels).
    -> {every: (hLambda, hMu, hDen)} float64 (nz, nx), summed over shot_ids (per_shot: a list with one such triple per shot), and
    the gathers (nshots, 4, nrec, nSteps) of the loop."""
    assert oracle.VARIANT == "", "pseudo_hessian_ref restates the unfused oracle build"
    L = oracle.lib()
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    Lambda, Mu, Den, Stf = f32(Lambda), f32(Mu), f32(Den), f32(Stf)
    ids = [int(i) for i in np.asarray(shot_ids).reshape(-1)]
    everies = tuple(int(e) for e in every)
    nz, nx, nSteps, nPml, nPad = [int(para[k]) for k in ("nz", "nx", "nSteps", "nPoints_pml", "nPad")]
    dz, dx, dt, f0 = [float(para[k]) for k in ("dz", "dx", "dt", "f0")]
    fiber = 1 if para.get("das_fiber", "horizontal") == "vertical" else 0
    fLam = f32((Lambda.T.astype(np.float64) * 1e6).astype(np.float32))   # transpose + MEGA through double, libCUFD.cu:71-77
    fMu = f32((Mu.T.astype(np.float64) * 1e6).astype(np.float32))
    fDen = f32(Den.T)
    Cp, aMu, bA, bB = [np.zeros((nx, nz), np.float32) for _ in range(4)]
    L.ofwi_model_average(_fp(fLam), _fp(fMu), _fp(fDen), C.c_int(nz), C.c_int(nx), _fp(Cp), _fp(aMu), _fp(bA), _fp(bB))
    nzc = nz - nPad
    cz, cx = np.zeros(6 * nzc, np.float32), np.zeros(6 * nx, np.float32)
    L.ofwi_cpml_init(*[_fp(cz[k * nzc:(k + 1) * nzc]) for k in range(6)], C.c_int(nzc), C.c_int(nPml), C.c_float(dz), C.c_float(f0), C.c_float(dt))
    L.ofwi_cpml_init(*[_fp(cx[k * nx:(k + 1) * nx]) for k in range(6)], C.c_int(nx), C.c_int(nPml), C.c_float(dx), C.c_float(f0), C.c_float(dt))
    prm = (nz, nx, nSteps, nPml, nPad, dz, dx, dt, fiber)
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
    for sid in ids:
        sh = survey["shot%d" % sid]
        assert "das_sensitivity" not in sh
        stf_s = oracle.window_stf(Stf[sid], dt)                       # Src_Rec.cu:130-137
        z_rec, x_rec = np.asarray(sh["z_rec"], np.int64) + nPml, np.asarray(sh["x_rec"], np.int64) + nPml
        E = {e: [np.zeros(shape, np.float64) for _ in range(3)] for e in everies}
        syn_all.append(_shot(L, prm, (fLam, fMu, aMu, bA, bB), cz, cx, stf_s, int(sh["z_src"]) + nPml, int(sh["x_src"]) + nPml, z_rec, x_rec,
                             everies, E))
        for e in everies:
            for k in range(3):
                total[e][k] += E[e][k]
        if per_shot:
            shots.append({e: dense(E[e]) for e in everies})
    out = {e: dense(total[e]) for e in everies}
    return (out, np.stack(syn_all), shots) if per_shot else (out, np.stack(syn_all))
