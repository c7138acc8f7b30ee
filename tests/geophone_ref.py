"""The reference for geophone (vx / vz) residuals in misfit and adjoint source (parameter keys misfit_w_*, csrc/geophone.hpp), shared by
every test that compares them with the CPU oracle.

The oracle's driver injects the axial strain only.  Its four stencil kernels and its helpers are exported, so this module is the
oracle's shot driver (ofwi_shot / ofwi_cufd, oracle/torchfwi_oracle.c:630-861) restated statement by statement as a Python step loop
over those functions, with ONE addition: after the axial-strain adds of a backward step,
    vx_adj(z, x) += w_vx r_vx        vz_adj(z, x) += w_vz r_vz        per channel, at the channel's own cell
(where the reference's res_injection_vx / _vz would add them, Src/utilities.cu:656-689), and
    misfit = 0.5 sum_shots ( w_ett sum r_ett^2 + w_vx sum r_vx^2 + w_vz sum r_vz^2 ),   the sums in float64.
With weights (1, 0, 0) it returns the oracle's gradients, gStf and gathers bit for bit (tests/test_geophone_reference.py): that pin
makes it a valid stand-in.  That pin holds on the default build (nothing fused); on the nvfma build, which exports the same kernels, the
loop is a second valid rounding of the same arithmetic (the yardstick of tests/test_gpu_born_fuzz.py)."""
import ctypes as C

import numpy as np


class _Cpml(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_float)) for n in ("K_z", "a_z", "b_z", "K_z_half", "a_z_half", "b_z_half",
                                                    "K_x", "a_x", "b_x", "K_x_half", "a_x_half", "b_x_half")]


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


def _shot(L, prm, media, cz, cx, stf, z_src, x_src, rxz, z_rec, x_rec, sens, calc_id, obs, weights, grads):
    """One shot (ofwi_shot).  Arrays are [x][z]; obs (4, nrec, nSteps) or None.  -> syn (4, nrec, nSteps), res or None, gStf or None."""
    nz, nx, nSteps, nPml, nPad, dz, dx, dt, fiber = prm
    fLam, fMu, aMu, bA, bB = media
    nzc = nz - nPad
    c = _Cpml(*([_fp(cz[k * nzc:(k + 1) * nzc]) for k in range(6)] + [_fp(cx[k * nx:(k + 1) * nx]) for k in range(6)]))
    dims = (C.c_int(nz), C.c_int(nx), C.c_float(dt), C.c_float(dz), C.c_float(dx), C.c_int(nPml), C.c_int(nPad))
    f = {k: np.zeros((nx, nz), np.float32) for k in ("vz", "vx", "szz", "sxx", "sxz", "vz_adj", "vx_adj", "szz_adj", "sxx_adj", "sxz_adj",
                                                     "dvz_dz", "dvz_dx", "dvx_dz", "dvx_dx", "dszz_dz", "dsxx_dx", "dsxz_dz", "dsxz_dx")}
    p = {k: _fp(v) for k, v in f.items()}
    with_adj, if_res = calc_id == 1, calc_id in (0, 1)
    nrec = z_rec.size
    w_ett, w_vx, w_vz = [np.float32(w) for w in weights]

    def stress(is_for, *img):
        L.ofwi_el_stress(p["vz"], p["vx"], p["szz"], p["sxx"], p["sxz"], p["dvz_dz"], p["dvz_dx"], p["dvx_dz"], p["dvx_dx"],
                         _fp(fLam), _fp(fMu), _fp(aMu), C.byref(c), *dims, C.c_int(is_for), *(img or (None,) * 5))

    def velocity(is_for, *img):
        L.ofwi_el_velocity(p["vz"], p["vx"], p["szz"], p["sxx"], p["sxz"], p["dszz_dz"], p["dsxz_dx"], p["dsxz_dz"], p["dsxx_dx"],
                           _fp(bA), _fp(bB), C.byref(c), *dims, C.c_int(is_for), *(img or (None,) * 3))

    adj_args = (p["vz_adj"], p["vx_adj"], p["szz_adj"], p["sxx_adj"], p["sxz_adj"], p["dszz_dz"], p["dsxz_dx"], p["dsxz_dz"], p["dsxx_dx"],
                p["dvz_dz"], p["dvz_dx"], p["dvx_dz"], p["dvx_dx"], _fp(fLam), _fp(fMu), _fp(aMu), _fp(bA), _fp(bB), C.byref(c)) + dims

    if with_adj:
        blen = L.ofwi_bnd_len(C.c_int(nz), C.c_int(nx), C.c_int(nPml), C.c_int(nPad))
        zmap, xmap = np.zeros(blen, np.int32), np.zeros(blen, np.int32)
        L.ofwi_bnd_map(C.c_int(nz), C.c_int(nx), C.c_int(nPml), C.c_int(nPad), zmap.ctypes.data_as(C.POINTER(C.c_int)),
                       xmap.ctypes.data_as(C.POINTER(C.c_int)))
        frames = {k: np.zeros((nSteps, blen), np.float32) for k in ("szz", "sxz", "sxx", "vz", "vx")}
    syn = np.zeros((4, nrec, nSteps), np.float32)
    src_scale = np.float32(1500.0 ** 2)                               # utilities.cu:531
    dxdz = np.float32(dx) / np.float32(dz)
    dtf = np.float32(dt)

    # ---- forward time loop, libCUFD.cu:268-332 ----
    for it in range(nSteps - 1):
        if with_adj:
            for k in ("szz", "sxz", "sxx", "vz", "vx"):
                frames[k][it] = f[k][xmap, zmap]
        stress(1)
        amp = np.float32(np.float32(src_scale * stf[it]) * dtf)       # add_source, utilities.cu:524-552
        f["szz"][x_src, z_src] = amp + f["szz"][x_src, z_src]
        f["sxx"][x_src, z_src] = amp + f["sxx"][x_src, z_src]
        velocity(1)
        vx, vz = f["vx"], f["vz"]
        syn[0, :, it + 1] = f["szz"][x_rec, z_rec] + f["sxx"][x_rec, z_rec]
        syn[1, :, it + 1] = vx[x_rec, z_rec]
        syn[2, :, it + 1] = vz[x_rec, z_rec]
        if sens is not None:                                          # das_directional
            exx = vx[x_rec, z_rec] - vx[x_rec - 1, z_rec]
            ezz = (vz[x_rec, z_rec] - vz[x_rec, z_rec - 1]) * dxdz
            exz = np.float32(0.5) * ((vx[x_rec, z_rec + 1] - vx[x_rec, z_rec]) * dxdz + (vz[x_rec + 1, z_rec] - vz[x_rec, z_rec]))
            syn[3, :, it + 1] = sens[:, 0] * exx + sens[:, 1] * ezz + sens[:, 2] * exz
        elif fiber:
            syn[3, :, it + 1] = vz[x_rec, z_rec] - vz[x_rec, z_rec - 1]
        else:
            syn[3, :, it + 1] = vx[x_rec, z_rec] - vx[x_rec - 1, z_rec]

    # ---- residuals, libCUFD.cu:410-427; gpuMinus utilities.cu:154-167 ----
    res = None
    if if_res:
        res = (obs - syn).astype(np.float32)
        res[:, :, 0] = 0.0
    if not with_adj:
        return syn, res, None

    # ---- backward, libCUFD.cu:500-675 ----
    gLam, gMu, gDen = grads
    gStf = np.zeros(nSteps, np.float32)
    for k in ("dvz_dz", "dvz_dx", "dvx_dz", "dvx_dx", "dszz_dz", "dsxx_dx", "dsxz_dz", "dsxz_dx"):
        f[k][:] = 0.0
    L.ofwi_el_velocity_adj(*adj_args)                                 # the two pre-loop launches on all-zero fields (:520-542)
    L.ofwi_el_stress_adj(*adj_args)
    flat = lambda xx, zz: (xx.astype(np.int64) * nz + zz).astype(np.int64)
    cell = flat(x_rec, z_rec)
    # per field the flat targets of one channel's adds in statement order (the values follow per step)
    if sens is not None:                                              # das_directional_adj
        ix_vx = np.stack([cell, flat(x_rec - 1, z_rec), flat(x_rec, z_rec + 1), cell], 1)
        ix_vz = np.stack([cell, flat(x_rec, z_rec - 1), flat(x_rec + 1, z_rec), cell], 1)
    elif fiber:
        ix_vx, ix_vz = np.zeros((nrec, 0), np.int64), np.stack([cell, flat(x_rec, z_rec - 1)], 1)
    else:
        ix_vx, ix_vz = np.stack([cell, flat(x_rec - 1, z_rec)], 1), np.zeros((nrec, 0), np.int64)
    if not w_ett > 0:
        ix_vx, ix_vz = ix_vx[:, :0], ix_vz[:, :0]
    if w_vx > 0:
        ix_vx = np.concatenate([ix_vx, cell[:, None]], 1)
    if w_vz > 0:
        ix_vz = np.concatenate([ix_vz, cell[:, None]], 1)
    vxa, vza = f["vx_adj"].reshape(-1), f["vz_adj"].reshape(-1)
    for it in range(nSteps - 2, -1, -1):
        # source_grad, utilities.cu:719-730
        gStf[it] = -np.float32((float(f["sxx_adj"][x_src, z_src]) * float(rxz) + float(f["szz_adj"][x_src, z_src])) * float(dtf))
        velocity(0, p["vz_adj"], p["vx_adj"], _fp(gDen))
        f["vz"][xmap, zmap] = frames["vz"][it]
        f["vx"][xmap, zmap] = frames["vx"][it]
        amp = np.float32(np.float32(src_scale * stf[it]) * dtf)
        f["szz"][x_src, z_src] -= amp
        f["sxx"][x_src, z_src] -= amp
        stress(0, p["szz_adj"], p["sxx_adj"], p["sxz_adj"], _fp(gLam), _fp(gMu))
        f["szz"][xmap, zmap] = frames["szz"][it]
        f["sxz"][xmap, zmap] = frames["sxz"][it]
        f["sxx"][xmap, zmap] = frames["sxx"][it]
        L.ofwi_el_velocity_adj(*adj_args)
        # res_injection_exx / _ezz / das_directional_adj per channel (utilities.cu:605-641), then the geophone adds of that channel
        rr = res[3, :, it]
        v_vx, v_vz = [], []
        if w_ett > 0:
            if w_ett != 1:
                rr = w_ett * rr
            if sens is not None:
                a, b, cc = sens[:, 0] * rr, sens[:, 1] * dxdz * rr, np.float32(0.5) * sens[:, 2] * rr
                v_vx, v_vz = [a, -a, cc * dxdz, -(cc * dxdz)], [b, -b, cc, -cc]
            elif fiber:
                v_vz = [rr, -rr]
            else:
                v_vx = [rr, -rr]
        if w_vx > 0:
            v_vx = v_vx + [w_vx * res[1, :, it]]
        if w_vz > 0:
            v_vz = v_vz + [w_vz * res[2, :, it]]
        if v_vx:
            np.add.at(vxa, ix_vx.ravel(), np.stack(v_vx, 1).astype(np.float32).ravel())
        if v_vz:
            np.add.at(vza, ix_vz.ravel(), np.stack(v_vz, 1).astype(np.float32).ravel())
        L.ofwi_el_stress_adj(*adj_args)
    return syn, res, gStf


def cufd(oracle, Lambda, Mu, Den, Stf, calc_id, shot_ids, para, survey, obs=None, weights=(1.0, 0.0, 0.0)):
    """The oracle's cufd call (oracle.cufd's arguments; no conditioning, no adj_src) with weights = (w_ett, w_vx, w_vz).
    -> dict(misfit, parts {vx, vz, ett: 0.5 sum r_c^2, float64}, gLambda, gMu, gDen, gStf, syn, res)."""
    L = oracle.lib()
    missing = [f for f in ("ofwi_el_stress", "ofwi_el_velocity", "ofwi_el_stress_adj", "ofwi_el_velocity_adj", "ofwi_model_average", "ofwi_cpml_init",
                           "ofwi_bnd_len", "ofwi_bnd_map") if not hasattr(L, f)]
    assert not missing, "this oracle build does not export %s" % ", ".join(missing)
    L.ofwi_bnd_len.restype = C.c_int
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    Lambda, Mu, Den, Stf = f32(Lambda), f32(Mu), f32(Den), f32(Stf)
    ids = [int(i) for i in np.asarray(shot_ids).reshape(-1)]
    nz, nx, nSteps, nPml, nPad = [int(para[k]) for k in ("nz", "nx", "nSteps", "nPoints_pml", "nPad")]
    dz, dx, dt, f0 = [float(para[k]) for k in ("dz", "dx", "dt", "f0")]
    fiber = 1 if para.get("das_fiber", "horizontal") == "vertical" else 0
    # transpose + MEGA through double, libCUFD.cu:71-77
    fLam = f32((Lambda.T.astype(np.float64) * 1e6).astype(np.float32))
    fMu = f32((Mu.T.astype(np.float64) * 1e6).astype(np.float32))
    fDen = f32(Den.T)
    Cp, aMu, bA, bB = [np.zeros((nx, nz), np.float32) for _ in range(4)]
    L.ofwi_model_average(_fp(fLam), _fp(fMu), _fp(fDen), C.c_int(nz), C.c_int(nx), _fp(Cp), _fp(aMu), _fp(bA), _fp(bB))
    nzc = nz - nPad
    cz, cx = np.zeros(6 * nzc, np.float32), np.zeros(6 * nx, np.float32)
    L.ofwi_cpml_init(*[_fp(cz[k * nzc:(k + 1) * nzc]) for k in range(6)], C.c_int(nzc), C.c_int(nPml), C.c_float(dz), C.c_float(f0), C.c_float(dt))
    L.ofwi_cpml_init(*[_fp(cx[k * nx:(k + 1) * nx]) for k in range(6)], C.c_int(nx), C.c_int(nPml), C.c_float(dx), C.c_float(f0), C.c_float(dt))
    prm = (nz, nx, nSteps, nPml, nPad, dz, dx, dt, fiber)
    with_adj = calc_id == 1
    syn_all, res_all, gstf_all, gbuf = [], [], [], []
    sums = np.zeros(4, np.float64)
    for i, sid in enumerate(ids):
        sh = survey["shot%d" % sid]
        stf_s = oracle.window_stf(Stf[sid], dt)                       # Src_Rec.cu:130-137
        z_rec, x_rec = np.asarray(sh["z_rec"], np.int64) + nPml, np.asarray(sh["x_rec"], np.int64) + nPml
        sens = None
        if "das_sensitivity" in sh:
            sens = f32(np.asarray(sh["das_sensitivity"], np.float64).reshape(z_rec.size, 6)[:, [0, 3, 1]])
        grads = [np.zeros((nx, nz), np.float32) for _ in range(3)] if with_adj else None
        syn, res, gstf = _shot(L, prm, (fLam, fMu, aMu, bA, bB), cz, cx, stf_s, int(sh["z_src"]) + nPml, int(sh["x_src"]) + nPml,
                               float(sh.get("src_rxz", 1.0)), z_rec, x_rec, sens, calc_id, None if obs is None else f32(obs[i]), weights, grads)
        syn_all.append(syn)
        if res is not None:
            res_all.append(res)
            sums += (res.astype(np.float64) ** 2).sum((1, 2))
        if with_adj:
            gstf_all.append(gstf)
            gbuf.append(grads)
    out = dict(syn=np.stack(syn_all))
    if res_all:
        w_ett, w_vx, w_vz = [float(np.float32(w)) for w in weights]
        out["res"] = np.stack(res_all)
        out["parts"] = dict(vx=0.5 * sums[1], vz=0.5 * sums[2], ett=0.5 * sums[3])
        out["misfit"] = 0.5 * (w_ett * sums[3] + w_vx * sums[1] + w_vz * sums[2])
    if with_adj:
        for k in range(1, len(gbuf)):                                 # reduced in shot order, as ofwi_cufd does
            for j in range(3):
                gbuf[0][j] += gbuf[k][j]
        out.update(gLambda=gbuf[0][0].T.copy(), gMu=gbuf[0][1].T.copy(), gDen=gbuf[0][2].T.copy(), gStf=np.stack(gstf_all))
    return out
