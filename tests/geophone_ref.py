"""The reference for geophone (vx / vz) residuals in misfit and adjoint source (parameter keys misfit_w_*, csrc/geophone.hpp), shared by
every test that compares them with the CPU oracle.

The oracle's driver injects the axial strain only.  Its four stencil kernels and its helpers are exported (tests/oracle_loop.py binds
them), so this module is the oracle's shot driver (ofwi_shot / ofwi_cufd, oracle/torchfwi_oracle.c:630-861) restated statement by
statement as a Python step loop over those functions, with ONE addition: after the axial-strain adds of a backward step,
    vx_adj(z, x) += w_vx r_vx        vz_adj(z, x) += w_vz r_vz        per channel, at the channel's own cell
(where the reference's res_injection_vx / _vz would add them, Src/utilities.cu:656-689), and
    misfit = 0.5 sum_shots ( w_ett sum r_ett^2 + w_vx sum r_vx^2 + w_vz sum r_vz^2 ),   the sums in float64.
With weights (1, 0, 0) it returns the oracle's gradients, gStf and gathers bit for bit (tests/test_geophone_reference.py): that pin
makes it a valid stand-in.  That pin holds on the default build (nothing fused); on the nvfma build, which exports the same kernels, the
loop is a second valid rounding of the same arithmetic (the yardstick of tests/test_gpu_born_fuzz.py)."""
import numpy as np

import oracle_loop as OL


def _shot(s, stf, z_src, x_src, rxz, z_rec, x_rec, sens, calc_id, obs, weights, grads):
    """One shot (ofwi_shot) of the call s (oracle_loop.Setup).  obs (4, nrec, nSteps) or None.  -> syn (4, nrec, nSteps), res or None, gStf or None."""
    nz, nSteps, fiber, dxdz, dtf = s.nz, s.nSteps, s.fiber, s.dxdz, s.dtf
    f = s.new_fields(OL.FIELDS + OL.ADJ + OL.MEM_S + OL.MEM_V)
    with_adj, if_res = calc_id == 1, calc_id in (0, 1)
    nrec = z_rec.size
    w_ett, w_vx, w_vz = [np.float32(w) for w in weights]
    if with_adj:
        zmap, xmap = s.boundary_map()
        frames = {k: np.zeros((nSteps, zmap.size), np.float32) for k in ("szz", "sxz", "sxx", "vz", "vx")}
    syn = np.zeros((4, nrec, nSteps), np.float32)

    # ---- forward time loop, libCUFD.cu:268-332 ----
    for it in range(nSteps - 1):
        if with_adj:
            for k in ("szz", "sxz", "sxx", "vz", "vx"):
                frames[k][it] = f[k][xmap, zmap]
        s.stress(f, s.fLam, s.fMu, s.aMu)
        s.add_source(f, stf[it], z_src, x_src)
        s.velocity(f, s.bA, s.bB)
        s.record(syn, it + 1, f, z_rec, x_rec, sens)

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
    s.velocity_adj(f)                                                 # the two pre-loop launches on all-zero fields (:520-542)
    s.stress_adj(f)
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
        s.velocity(f, s.bA, s.bB, 0, [f["vz_adj"], f["vx_adj"], gDen])
        f["vz"][xmap, zmap] = frames["vz"][it]
        f["vx"][xmap, zmap] = frames["vx"][it]
        amp = s.source_amp(stf[it])
        f["szz"][x_src, z_src] -= amp
        f["sxx"][x_src, z_src] -= amp
        s.stress(f, s.fLam, s.fMu, s.aMu, 0, [f["szz_adj"], f["sxx_adj"], f["sxz_adj"], gLam, gMu])
        f["szz"][xmap, zmap] = frames["szz"][it]
        f["sxz"][xmap, zmap] = frames["sxz"][it]
        f["sxx"][xmap, zmap] = frames["sxx"][it]
        s.velocity_adj(f)
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
        s.stress_adj(f)
    return syn, res, gStf


def cufd(oracle, Lambda, Mu, Den, Stf, calc_id, shot_ids, para, survey, obs=None, weights=(1.0, 0.0, 0.0)):
    """The oracle's cufd call (oracle.cufd's arguments; no conditioning, no adj_src) with weights = (w_ett, w_vx, w_vz).
    -> dict(misfit, parts {vx, vz, ett: 0.5 sum r_c^2, float64}, gLambda, gMu, gDen, gStf, syn, res)."""
    s = OL.Setup(oracle, Lambda, Mu, Den, para, OL.FORWARD + OL.BACKWARD)
    with_adj = calc_id == 1
    syn_all, res_all, gstf_all, gbuf = [], [], [], []
    sums = np.zeros(4, np.float64)
    for i, (sid, stf_s, z_src, x_src, z_rec, x_rec, rxz, sens) in enumerate(s.shots(Stf, shot_ids, survey)):
        grads = [np.zeros((s.nx, s.nz), np.float32) for _ in range(3)] if with_adj else None
        syn, res, gstf = _shot(s, stf_s, z_src, x_src, rxz, z_rec, x_rec, sens, calc_id, None if obs is None else OL.f32(obs[i]), weights, grads)
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
