"""The reference for Born modelling (csrc/born.hpp, sepfwi_born), shared by every test that compares it with the CPU oracle.

The reference package has nothing of the kind, so this is an unpinned extension.  The oracle's stencil kernels and helpers are
exported and take the media as arguments; they are linear in the fields, and linear in the media when the updated field starts at
zero.  So the scattered step needs no new C: this module is the oracle's forward shot loop (ofwi_shot, oracle/torchfwi_oracle.c)
restated as a Python step loop over ofwi_el_stress / ofwi_el_velocity / ofwi_model_average / ofwi_cpml_init exactly as
pseudo_hessian_ref._shot does it, and per half-step
    (a) coupling term     the kernel on COPIES of the background's input fields and of its four C-PML memories of that half-step (taken
                          before the background half-step changes them), with the perturbed media (dlam, dmu, damu) resp. (dba, dbb) and
                          zeroed output fields: the output is the coupling term, with the background's C-PML-modified derivatives
    (b) propagation term  the kernel on the scattered fields (their own eight memories) with the background media
and (a) is added to the result of (b).  No source term.  The background loop's gathers equal oracle.cufd(..., calc_id 2) bit for bit
(tests/test_born_reference.py), which makes it the oracle's loop; the scattered gathers are confirmed there against central finite
differences of the oracle's gathers.

Perturbed media, float64 numpy from the oracle's own aMu, bA, bB (arrays [x][z]), cast to float32, zero outside [2, n-3]^2:
    dlam = 1e6 dLambda, dmu = 1e6 dMu
    damu = (aMu^2 / 4) sum_k dmu_k / mu_k^2  over (z,x), (z+1,x), (z,x+1), (z+1,x+1);  0 where aMu is 0
    dba  = -(bA^2 / 2) (dDen(z+1,x) + dDen(z,x)),   dbb = -(bB^2 / 2) (dDen(z,x+1) + dDen(z,x))
Either oracle build serves: both export the same kernels and helpers, and the loop run on the nvfma build (the reference binary's fused
multiply-adds inside the kernels) is a second valid rounding of the same arithmetic -- the yardstick of the fuzz tests."""
import ctypes as C

import numpy as np

from geophone_ref import _Cpml, _fp

EXPORTS = ("ofwi_el_stress", "ofwi_el_velocity", "ofwi_model_average", "ofwi_cpml_init")      # what the loop needs of an oracle build
FIELDS = ("vz", "vx", "szz", "sxx", "sxz")
MEM_S = ("dvz_dz", "dvz_dx", "dvx_dz", "dvx_dx")          # written by the stress kernel
MEM_V = ("dszz_dz", "dsxz_dx", "dsxz_dz", "dsxx_dx")      # written by the velocity kernel

f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def internal_media(oracle, Lambda, Mu, Den, nz, nx):
    """(fLam, fMu, fDen, aMu, bA, bB), arrays [x][z]: transpose + MEGA through double (libCUFD.cu:71-77), ofwi_model_average."""
    L = oracle.lib()
    fLam = f32((f32(Lambda).T.astype(np.float64) * 1e6).astype(np.float32))
    fMu = f32((f32(Mu).T.astype(np.float64) * 1e6).astype(np.float32))
    fDen = f32(f32(Den).T)
    Cp, aMu, bA, bB = [np.zeros((nx, nz), np.float32) for _ in range(4)]
    L.ofwi_model_average(_fp(fLam), _fp(fMu), _fp(fDen), C.c_int(nz), C.c_int(nx), _fp(Cp), _fp(aMu), _fp(bA), _fp(bB))
    return fLam, fMu, fDen, aMu, bA, bB


def delta_media(media, dLambda, dMu, dDen):
    """The five perturbed-media arrays [x][z] float32 (module docstring) from internal_media's tuple and dense (nz, nx) v."""
    fLam, fMu, fDen, aMu, bA, bB = media
    nx, nz = fMu.shape
    dlam = (f32(dLambda).T.astype(np.float64) * 1e6)
    dmu = (f32(dMu).T.astype(np.float64) * 1e6)
    dden = f32(dDen).T.astype(np.float64)
    damu, dba, dbb = [np.zeros((nx, nz), np.float64) for _ in range(3)]
    xs, zs = slice(2, nx - 2), slice(2, nz - 2)
    sh = lambda a, kx, kz: a[xs.start + kx:xs.stop + kx, zs.start + kz:zs.stop + kz]
    mu64 = fMu.astype(np.float64)
    am = aMu[xs, zs].astype(np.float64)
    s = np.zeros_like(am)
    with np.errstate(divide="ignore", invalid="ignore"):
        for kx, kz in ((0, 0), (0, 1), (1, 0), (1, 1)):
            s += np.where(am != 0.0, sh(dmu, kx, kz) / sh(mu64, kx, kz) ** 2, 0.0)
    damu[xs, zs] = np.where(am != 0.0, am * am / 4.0 * s, 0.0)
    dba[xs, zs] = -(bA[xs, zs].astype(np.float64) ** 2) / 2.0 * (sh(dden, 0, 1) + sh(dden, 0, 0))
    dbb[xs, zs] = -(bB[xs, zs].astype(np.float64) ** 2) / 2.0 * (sh(dden, 1, 0) + sh(dden, 0, 0))
    return f32(dlam), f32(dmu), f32(damu), f32(dba), f32(dbb)


def _sample(f, x_rec, z_rec, sens, fiber, dxdz):
    """The four samples (pr, vx, vz, ett) of one field set at the channels: the oracle's recording statements (linear in the fields)."""
    vx, vz = f["vx"], f["vz"]
    out = [f["szz"][x_rec, z_rec] + f["sxx"][x_rec, z_rec], vx[x_rec, z_rec], vz[x_rec, z_rec]]
    if sens is not None:                                          # das_directional
        exx = vx[x_rec, z_rec] - vx[x_rec - 1, z_rec]
        ezz = (vz[x_rec, z_rec] - vz[x_rec, z_rec - 1]) * dxdz
        exz = np.float32(0.5) * ((vx[x_rec, z_rec + 1] - vx[x_rec, z_rec]) * dxdz + (vz[x_rec + 1, z_rec] - vz[x_rec, z_rec]))
        out.append(sens[:, 0] * exx + sens[:, 1] * ezz + sens[:, 2] * exz)
    elif fiber:
        out.append(vz[x_rec, z_rec] - vz[x_rec, z_rec - 1])
    else:
        out.append(vx[x_rec, z_rec] - vx[x_rec - 1, z_rec])
    return out


def _shot(L, prm, media, dmedia, cz, cx, stf, z_src, x_src, z_rec, x_rec, sens, terms=(True, True, True)):
    """Forward loop of one shot, background and scattered field.  -> syn, dsyn (4, nrec, nSteps) each.
    terms: switches for the (lam/mu, amu, density) coupling terms -- all on, except in tests that show what a dropped term costs."""
    nz, nx, nSteps, nPml, nPad, dz, dx, dt, fiber = prm
    fLam, fMu, aMu, bA, bB = media
    dlam, dmu, damu, dba, dbb = dmedia
    zero = np.zeros((nx, nz), np.float32)
    if not terms[0]:
        dlam, dmu = zero, zero
    if not terms[1]:
        damu = zero
    if not terms[2]:
        dba, dbb = zero, zero
    nzc = nz - nPad
    c = _Cpml(*([_fp(cz[k * nzc:(k + 1) * nzc]) for k in range(6)] + [_fp(cx[k * nx:(k + 1) * nx]) for k in range(6)]))
    dims = (C.c_int(nz), C.c_int(nx), C.c_float(dt), C.c_float(dz), C.c_float(dx), C.c_int(nPml), C.c_int(nPad))
    new = lambda: {k: np.zeros((nx, nz), np.float32) for k in FIELDS + MEM_S + MEM_V}
    f, d, t = new(), new(), new()      # background, scattered, the coupling term's scratch set

    def stress(a, lam, mu, amu):
        L.ofwi_el_stress(_fp(a["vz"]), _fp(a["vx"]), _fp(a["szz"]), _fp(a["sxx"]), _fp(a["sxz"]), *[_fp(a[k]) for k in MEM_S],
                         _fp(lam), _fp(mu), _fp(amu), C.byref(c), *dims, C.c_int(1), *((None,) * 5))

    def velocity(a, ba, bb):
        L.ofwi_el_velocity(_fp(a["vz"]), _fp(a["vx"]), _fp(a["szz"]), _fp(a["sxx"]), _fp(a["sxz"]), *[_fp(a[k]) for k in MEM_V],
                           _fp(ba), _fp(bb), C.byref(c), *dims, C.c_int(1), *((None,) * 3))

    syn = np.zeros((4, z_rec.size, nSteps), np.float32)
    dsyn = np.zeros_like(syn)
    src_scale, dtf = np.float32(1500.0 ** 2), np.float32(dt)
    dxdz = np.float32(dx) / np.float32(dz)
    for it in range(nSteps - 1):
        # ---- stress half-step: (a) on copies of the background's velocities and stress-side memories, (b), then the background
        for k in ("vz", "vx") + MEM_S:
            t[k][:] = f[k]
        for k in ("szz", "sxx", "sxz"):
            t[k][:] = 0.0
        stress(t, dlam, dmu, damu)
        stress(d, fLam, fMu, aMu)
        for k in ("szz", "sxx", "sxz"):
            d[k] += t[k]
        stress(f, fLam, fMu, aMu)
        amp = np.float32(np.float32(src_scale * stf[it]) * dtf)       # add_source, utilities.cu:524-552 (the background only)
        f["szz"][x_src, z_src] = amp + f["szz"][x_src, z_src]
        f["sxx"][x_src, z_src] = amp + f["sxx"][x_src, z_src]
        # ---- velocity half-step: the background's stresses after update and source add
        for k in ("szz", "sxx", "sxz") + MEM_V:
            t[k][:] = f[k]
        for k in ("vz", "vx"):
            t[k][:] = 0.0
        velocity(t, dba, dbb)
        velocity(d, bA, bB)
        for k in ("vz", "vx"):
            d[k] += t[k]
        velocity(f, bA, bB)
        for k, v in enumerate(_sample(f, x_rec, z_rec, sens, fiber, dxdz)):
            syn[k, :, it + 1] = v
        for k, v in enumerate(_sample(d, x_rec, z_rec, sens, fiber, dxdz)):
            dsyn[k, :, it + 1] = v
    return syn, dsyn


def born(oracle, Lambda, Mu, Den, dLambda, dMu, dDen, Stf, shot_ids, para, survey, terms=(True, True, True), stack=True):
    """oracle.cufd's model arguments plus the perturbation (dense (nz, nx) each).  One-cell horizontal or vertical channels and
    directional ones (no gauge length: tests expand gauges into their member channels).
    -> dict(syn, dsyn: (nshots, 4, nrec, nSteps) background and scattered gathers [pr, vx, vz, ett]; dmedia: the five arrays [x][z]).
    stack=False: syn and dsyn are lists with one (4, nrec, nSteps) array per shot -- the shots may then have different channel counts."""
    L = oracle.lib()
    missing = [f for f in EXPORTS if not hasattr(L, f)]
    assert not missing, "this oracle build does not export %s" % ", ".join(missing)
    Stf = f32(Stf)
    ids = [int(i) for i in np.asarray(shot_ids).reshape(-1)]
    nz, nx, nSteps, nPml, nPad = [int(para[k]) for k in ("nz", "nx", "nSteps", "nPoints_pml", "nPad")]
    dz, dx, dt, f0 = [float(para[k]) for k in ("dz", "dx", "dt", "f0")]
    fiber = 1 if para.get("das_fiber", "horizontal") == "vertical" else 0
    med = internal_media(oracle, Lambda, Mu, Den, nz, nx)
    dmed = delta_media(med, dLambda, dMu, dDen)
    fLam, fMu, fDen, aMu, bA, bB = med
    nzc = nz - nPad
    cz, cx = np.zeros(6 * nzc, np.float32), np.zeros(6 * nx, np.float32)
    L.ofwi_cpml_init(*[_fp(cz[k * nzc:(k + 1) * nzc]) for k in range(6)], C.c_int(nzc), C.c_int(nPml), C.c_float(dz), C.c_float(f0), C.c_float(dt))
    L.ofwi_cpml_init(*[_fp(cx[k * nx:(k + 1) * nx]) for k in range(6)], C.c_int(nx), C.c_int(nPml), C.c_float(dx), C.c_float(f0), C.c_float(dt))
    prm = (nz, nx, nSteps, nPml, nPad, dz, dx, dt, fiber)
    syn_all, dsyn_all = [], []
    for sid in ids:
        sh = survey["shot%d" % sid]
        stf_s = oracle.window_stf(Stf[sid], dt)                       # Src_Rec.cu:130-137
        z_rec, x_rec = np.asarray(sh["z_rec"], np.int64) + nPml, np.asarray(sh["x_rec"], np.int64) + nPml
        sens = None
        if "das_sensitivity" in sh:
            sens = f32(np.asarray(sh["das_sensitivity"], np.float64).reshape(z_rec.size, 6)[:, [0, 3, 1]])
        syn, dsyn = _shot(L, prm, (fLam, fMu, aMu, bA, bB), dmed, cz, cx, stf_s, int(sh["z_src"]) + nPml, int(sh["x_src"]) + nPml, z_rec, x_rec,
                          sens, terms)
        syn_all.append(syn)
        dsyn_all.append(dsyn)
    if not stack:
        return dict(syn=syn_all, dsyn=dsyn_all, dmedia=dmed)
    return dict(syn=np.stack(syn_all), dsyn=np.stack(dsyn_all), dmedia=dmed)


def perturbation(pb, seed=3, scale=0.01, only=None, model="lame_init"):
    """A smooth random v = (dLambda, dMu, dDen) over the whole padded grid (PML included), about `scale` of the model's size, every
    parameter non-zero; only = 0 / 1 / 2: that parameter alone.  float32 numpy (nz, nx)."""
    import problems as P
    rng = np.random.default_rng(seed)
    out = []
    for k, m in enumerate(pb[model]):
        m = m.numpy()
        a = P.smooth_random(rng, m.shape, -1.0, 1.0, passes=6) * scale * float(np.abs(m).mean())
        out.append(f32(a if only is None or only == k else np.zeros_like(a)))
    return out


def born_fuzz_perturbation(pb, seed, water_rows):
    """perturbation(pb, seed) for a fuzz draw with `water_rows` rows of water on top (0: none): dMu is zero in the water rows -- a fluid
    stays a fluid (the harmonic mean of mu is not differentiable at mu = 0), as in test_born_reference.perturbation."""
    v = perturbation(pb, seed=seed)
    v[1][:int(water_rows)] = 0.0
    return v
