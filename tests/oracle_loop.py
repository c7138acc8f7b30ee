"""The one ctypes binding of the CPU oracle's exported stencil kernels and helpers (oracle/torchfwi_oracle.c), shared by the reference
modules that restate the oracle's shot loop as a Python step loop: geophone_ref, pseudo_hessian_ref and born_ref.  Each of them keeps its
own loop -- what it inserts between the half-steps is its reason to exist -- and takes from here everything the three share: the call's
set-up (Setup), the kernel calls on a field set, the source add, the recording statements and the survey read-out per shot.

Arrays are [x][z] float32.  Either oracle build serves: both export the same kernels, and a loop run on the nvfma build (the reference
binary's fused multiply-adds inside the kernels) is a second valid rounding of the same arithmetic, the yardstick of the fuzz tests."""
import ctypes as C

import numpy as np

FIELDS = ("vz", "vx", "szz", "sxx", "sxz")
MEM_S = ("dvz_dz", "dvz_dx", "dvx_dz", "dvx_dx")          # written by the stress kernel
MEM_V = ("dszz_dz", "dsxz_dx", "dsxz_dz", "dsxx_dx")      # written by the velocity kernel
ADJ = tuple(k + "_adj" for k in FIELDS)
FORWARD = ("ofwi_el_stress", "ofwi_el_velocity", "ofwi_model_average", "ofwi_cpml_init")      # what a forward loop needs of an oracle build
BACKWARD = ("ofwi_el_stress_adj", "ofwi_el_velocity_adj", "ofwi_bnd_len", "ofwi_bnd_map")

f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


class Cpml(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_float)) for n in ("K_z", "a_z", "b_z", "K_z_half", "a_z_half", "b_z_half",
                                                    "K_x", "a_x", "b_x", "K_x_half", "a_x_half", "b_x_half")]


def internal_media(oracle, Lambda, Mu, Den, nz, nx):
    """(fLam, fMu, fDen, aMu, bA, bB), arrays [x][z]: transpose + MEGA through double (libCUFD.cu:71-77), ofwi_model_average."""
    fLam = f32((f32(Lambda).T.astype(np.float64) * 1e6).astype(np.float32))
    fMu = f32((f32(Mu).T.astype(np.float64) * 1e6).astype(np.float32))
    fDen = f32(f32(Den).T)
    Cp, aMu, bA, bB = [np.zeros((nx, nz), np.float32) for _ in range(4)]
    oracle.lib().ofwi_model_average(fp(fLam), fp(fMu), fp(fDen), C.c_int(nz), C.c_int(nx), fp(Cp), fp(aMu), fp(bA), fp(bB))
    return fLam, fMu, fDen, aMu, bA, bB


class Setup:
    """What one call shares over its shots: the library handle L, the grid (nz, nx, nzc, nSteps, nPml, nPad, dz, dx, dt, fiber), the
    internal media fLam, fMu, fDen, aMu, bA, bB, and the C-PML coefficients behind the kernels' last arguments."""

    def __init__(self, oracle, Lambda, Mu, Den, para, exports=FORWARD):
        self.oracle, self.L = oracle, oracle.lib()
        missing = [f for f in exports if not hasattr(self.L, f)]
        assert not missing, "this oracle build does not export %s" % ", ".join(missing)
        nz, nx, self.nSteps, nPml, nPad = [int(para[k]) for k in ("nz", "nx", "nSteps", "nPoints_pml", "nPad")]
        dz, dx, dt, f0 = [float(para[k]) for k in ("dz", "dx", "dt", "f0")]
        self.nz, self.nx, self.nPml, self.nPad, self.dz, self.dx, self.dt = nz, nx, nPml, nPad, dz, dx, dt
        self.fiber = 1 if para.get("das_fiber", "horizontal") == "vertical" else 0
        self.media = internal_media(oracle, Lambda, Mu, Den, nz, nx)
        self.fLam, self.fMu, self.fDen, self.aMu, self.bA, self.bB = self.media
        self.nzc = nzc = nz - nPad
        self.cz, self.cx = np.zeros(6 * nzc, np.float32), np.zeros(6 * nx, np.float32)
        for c, n, h in ((self.cz, nzc, dz), (self.cx, nx, dx)):
            self.L.ofwi_cpml_init(*[fp(c[k * n:(k + 1) * n]) for k in range(6)], C.c_int(n), C.c_int(nPml), C.c_float(h), C.c_float(f0), C.c_float(dt))
        self.c = Cpml(*([fp(self.cz[k * nzc:(k + 1) * nzc]) for k in range(6)] + [fp(self.cx[k * nx:(k + 1) * nx]) for k in range(6)]))
        self.dims = (C.c_int(nz), C.c_int(nx), C.c_float(dt), C.c_float(dz), C.c_float(dx), C.c_int(nPml), C.c_int(nPad))
        self.src_scale, self.dtf = np.float32(1500.0 ** 2), np.float32(dt)      # utilities.cu:531
        self.dxdz = np.float32(dx) / np.float32(dz)

    def new_fields(self, names=FIELDS + MEM_S + MEM_V):
        return {k: np.zeros((self.nx, self.nz), np.float32) for k in names}

    def stress(self, a, lam, mu, amu, is_for=1, img=None):
        """ofwi_el_stress on the field set a with the media given; img: [szz_adj, sxx_adj, sxz_adj, gLam, gMu] of the imaging condition"""
        self.L.ofwi_el_stress(*[fp(a[k]) for k in FIELDS + MEM_S], fp(lam), fp(mu), fp(amu), C.byref(self.c), *self.dims, C.c_int(is_for),
                              *[fp(g) for g in img or (None,) * 5])

    def velocity(self, a, ba, bb, is_for=1, img=None):
        """ofwi_el_velocity on the field set a with the media given; img: [vz_adj, vx_adj, gDen] of the imaging condition"""
        self.L.ofwi_el_velocity(*[fp(a[k]) for k in FIELDS + MEM_V], fp(ba), fp(bb), C.byref(self.c), *self.dims, C.c_int(is_for),
                                *[fp(g) for g in img or (None,) * 3])

    def _adj_args(self, a):
        return [fp(a[k]) for k in ADJ + MEM_V + MEM_S] + [fp(m) for m in (self.fLam, self.fMu, self.aMu, self.bA, self.bB)] + [C.byref(self.c), *self.dims]

    def velocity_adj(self, a):
        self.L.ofwi_el_velocity_adj(*self._adj_args(a))

    def stress_adj(self, a):
        self.L.ofwi_el_stress_adj(*self._adj_args(a))

    def boundary_map(self):
        """(zmap, xmap) of the boundary frames that the backward loop restores (ofwi_bnd_map)"""
        size = [C.c_int(v) for v in (self.nz, self.nx, self.nPml, self.nPad)]
        self.L.ofwi_bnd_len.restype = C.c_int
        zmap, xmap = [np.zeros(self.L.ofwi_bnd_len(*size), np.int32) for _ in range(2)]
        self.L.ofwi_bnd_map(*size, zmap.ctypes.data_as(C.POINTER(C.c_int)), xmap.ctypes.data_as(C.POINTER(C.c_int)))
        return zmap, xmap

    def source_amp(self, s):
        """the amplitude that one source sample adds to szz and sxx (add_source, utilities.cu:524-552)"""
        return np.float32(np.float32(self.src_scale * s) * self.dtf)

    def add_source(self, a, s, z_src, x_src):
        amp = self.source_amp(s)
        a["szz"][x_src, z_src] = amp + a["szz"][x_src, z_src]
        a["sxx"][x_src, z_src] = amp + a["sxx"][x_src, z_src]

    def sample(self, a, z_rec, x_rec, sens):
        """The four rows [pr, vx, vz, ett] of one field set at the channels: the oracle's recording statements (linear in the fields)."""
        vx, vz, dxdz = a["vx"], a["vz"], self.dxdz
        out = [a["szz"][x_rec, z_rec] + a["sxx"][x_rec, z_rec], vx[x_rec, z_rec], vz[x_rec, z_rec]]
        if sens is not None:                                          # das_directional
            exx = vx[x_rec, z_rec] - vx[x_rec - 1, z_rec]
            ezz = (vz[x_rec, z_rec] - vz[x_rec, z_rec - 1]) * dxdz
            exz = np.float32(0.5) * ((vx[x_rec, z_rec + 1] - vx[x_rec, z_rec]) * dxdz + (vz[x_rec + 1, z_rec] - vz[x_rec, z_rec]))
            out.append(sens[:, 0] * exx + sens[:, 1] * ezz + sens[:, 2] * exz)
        elif self.fiber:
            out.append(vz[x_rec, z_rec] - vz[x_rec, z_rec - 1])
        else:
            out.append(vx[x_rec, z_rec] - vx[x_rec - 1, z_rec])
        return out

    def record(self, syn, it, a, z_rec, x_rec, sens):
        for k, v in enumerate(self.sample(a, z_rec, x_rec, sens)):
            syn[k, :, it] = v

    def shots(self, Stf, shot_ids, survey):
        """Per shot of the call: (shot id, windowed source trace, z_src, x_src, z_rec, x_rec (padded cells), src_rxz, sensitivities
        (nrec, 3) [xx, zz, xz] or None)."""
        Stf = f32(Stf)
        for sid in [int(i) for i in np.asarray(shot_ids).reshape(-1)]:
            sh = survey["shot%d" % sid]
            z_rec, x_rec = np.asarray(sh["z_rec"], np.int64) + self.nPml, np.asarray(sh["x_rec"], np.int64) + self.nPml
            sens = None
            if "das_sensitivity" in sh:
                sens = f32(np.asarray(sh["das_sensitivity"], np.float64).reshape(z_rec.size, 6)[:, [0, 3, 1]])
            yield (sid, self.oracle.window_stf(Stf[sid], self.dt), int(sh["z_src"]) + self.nPml, int(sh["x_src"]) + self.nPml,      # Src_Rec.cu:130-137
                   z_rec, x_rec, float(sh.get("src_rxz", 1.0)), sens)
