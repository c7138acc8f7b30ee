// born.hip -- the kernels of Born modelling (born.hpp).  A translation unit of its own: the field kernels (kernels.hip) are untouched.
// Bundle unpacking (kernels_device.hpp) and the launch tiling (tiled(), kernels.hpp) are the field kernels' own.
//
// k_born_stress / k_born_velocity have the launch shape and the cell mapping of k_stress / k_velocity (one wave per 64-column row
// segment, my_cell).  Each advances the BACKGROUND by calling the forward body (stress_body / velocity_body, kernels_bodies.hpp: the
// same inline code compiled with the same flags, so the background is bit for bit a plain forward pass) and the SCATTERED field next to
// it.  The scattered update needs the background's C-PML-modified derivatives of this very step: they are formed here from the same
// taps and the same expressions as in the body, before the body's first store -- the loads are the body's own (the compiler merges
// them: one round trip per wave, every load of the cell before its first store), the values are the body's bits.
#include <hip/hip_runtime.h>

#include "born.hpp"
#include "device_common.hpp"

namespace sepfwi {
#include "kernels_device.hpp"
#include "kernels_bodies.hpp"

namespace {

// The eight C-PML memories of a state bundle [5 fields | 8 memories].  Kept beside the kernels, like the region and strip tests
// written out in them: mem_of(b + 5 n, n), on_region and strip_xs / strip_xv (kernels_device.hpp) say the same, but with them the
// compiler schedules k_born_stress / k_born_velocity differently, and their instruction text is held fixed.
__device__ __forceinline__ PmlMem b_mem(float *b, size_t n) {
    return PmlMem{b + 5 * n, b + 6 * n, b + 7 * n, b + 8 * n, b + 9 * n, b + 10 * n, b + 11 * n, b + 12 * n};
}

// the four velocity derivatives of the stress update at cell i (the expressions of stress_body)
struct StressD {
    float vz_z, vx_x, vx_z, vz_x;
};
__device__ __forceinline__ StressD stress_derivs(const Grid &g, const Fields &f, size_t i) {
    const int P = g.pitch;
    const float vz0 = f.vz[i], vx0 = f.vx[i];
    StressD d;
    d.vz_z = dminus(f.vz[i - 2 * P], f.vz[i - P], vz0, f.vz[i + P], g.rdz);
    d.vx_x = dminus(f.vx[i - 2], f.vx[i - 1], vx0, f.vx[i + 1], g.rdx);
    d.vx_z = dplus(f.vx[i - P], vx0, f.vx[i + P], f.vx[i + 2 * P], g.rdz);
    d.vz_x = dplus(f.vz[i - 1], vz0, f.vz[i + 1], f.vz[i + 2], g.rdx);
    return d;
}
// the four stress derivatives of the velocity update at cell i (the expressions of velocity_body)
struct VelD {
    float szz_z, sxz_x, sxz_z, sxx_x;
};
__device__ __forceinline__ VelD velocity_derivs(const Grid &g, const Fields &f, size_t i) {
    const int P = g.pitch;
    VelD d;
    d.szz_z = dplus(f.szz[i - P], f.szz[i], f.szz[i + P], f.szz[i + 2 * P], g.rdz);
    d.sxz_x = dminus(f.sxz[i - 2], f.sxz[i - 1], f.sxz[i], f.sxz[i + 1], g.rdx);
    d.sxz_z = dminus(f.sxz[i - 2 * P], f.sxz[i - P], f.sxz[i], f.sxz[i + P], g.rdz);
    d.sxx_x = dplus(f.sxx[i - 1], f.sxx[i], f.sxx[i + 1], f.sxx[i + 2], g.rdx);
    return d;
}

}  // namespace

// SRC: the scattered field has a source term of its own (a perturbation ds of the source time function: dsrc_amp = scale T ds[it] dt,
// added to dszz and dsxx of the source cell where the background gets src_amp).  Without one the instance adds nothing -- not even a
// +0.0f, which would turn a -0 into +0.
template <bool SAVE, bool SRC>
__global__ __launch_bounds__(MAXT) void k_born_stress(Grid g, BornArgs b, float *__restrict__ frame_t, int zx_src /* z<<16 | x */, float src_amp,
                                                      float dsrc_amp) {
    const Fields f = fields_of(b.state, b.n), df = fields_of(b.dstate, b.n);
    const PmlMem m = b_mem(b.state, b.n), dm = b_mem(b.dstate, b.n);
    const Media md = media_of(b.media, b.n);
    const PmlCoef pc = coef_of(b.cz, b.cz + 6 * g.nzc, g.nzc, g.nx);
    const Cell c = my_cell(g);
    const int z = c.z, x = c.x;
    const size_t i = c.i;
    // the update region of the forward body (el_stress.cu:52)
    const bool on = !(z >= g.nzc || x >= g.nx || z < 2 || z > g.nzc - 3 || x < 2 || x > g.nx - 3);
    const bool pz = on && in_pml_z(g, z);                             // wave-uniform
    const bool px = on && (x < g.nPml || x > g.nx - g.nPml - 1);      // el_stress.cu:61,77
    StressD D{}, E{};  // background, scattered
    float lam = 0.f, mu = 0.f, amu = 0.f, dlam = 0.f, dmu = 0.f, damu = 0.f, dszz0 = 0.f, dsxx0 = 0.f, dsxz0 = 0.f;
    float e_p = 0.f, e_q = 0.f, e_r = 0.f, e_s = 0.f;
    if (on) {
        // every load of the cell, background and scattered, before the first store
        D = stress_derivs(g, f, i);
        E = stress_derivs(g, df, i);
        lam = md.lam[i];
        mu = md.mu[i];
        amu = ave_mu_at(g, md, i, mu);
        dlam = b.dmedia[i];
        dmu = b.dmedia[b.n + i];
        damu = b.dmedia[2 * b.n + i];
        dszz0 = df.szz[i];
        dsxx0 = df.sxx[i];
        dsxz0 = df.sxz[i];
        if (pz) {  // the recursion of the body on the background's memories as they stand, and on the scattered field's own
            const float p = pc.b_z[z] * m.dvz_dz[i] + pc.a_z[z] * D.vz_z;
            D.vz_z = D.vz_z * pc.rK_z[z] + p;
            const float q = pc.b_zh[z] * m.dvx_dz[i] + pc.a_zh[z] * D.vx_z;
            D.vx_z = D.vx_z * pc.rK_zh[z] + q;
            e_p = pc.b_z[z] * dm.dvz_dz[i] + pc.a_z[z] * E.vz_z;
            E.vz_z = E.vz_z * pc.rK_z[z] + e_p;
            e_q = pc.b_zh[z] * dm.dvx_dz[i] + pc.a_zh[z] * E.vx_z;
            E.vx_z = E.vx_z * pc.rK_zh[z] + e_q;
        }
        if (px) {
            const float p = pc.b_x[x] * m.dvx_dx[i] + pc.a_x[x] * D.vx_x;
            D.vx_x = D.vx_x * pc.rK_x[x] + p;
            const float q = pc.b_xh[x] * m.dvz_dx[i] + pc.a_xh[x] * D.vz_x;
            D.vz_x = D.vz_x * pc.rK_xh[x] + q;
            e_r = pc.b_x[x] * dm.dvx_dx[i] + pc.a_x[x] * E.vx_x;
            E.vx_x = E.vx_x * pc.rK_x[x] + e_r;
            e_s = pc.b_xh[x] * dm.dvz_dx[i] + pc.a_xh[x] * E.vz_x;
            E.vz_x = E.vz_x * pc.rK_xh[x] + e_s;
        }
    }
    // the background: the forward body itself (boundary-frame save, update, source add)
    stress_body<true, SAVE>(g, c, f, m, md, pc, frame_t, zx_src >> 16, zx_src & 0xffff, src_amp, Fields{}, AccG{}, LineRec{});
    if (!on) return;
    if (pz) {
        dm.dvz_dz[i] = e_p;
        dm.dvx_dz[i] = e_q;
    }
    if (px) {
        dm.dvx_dx[i] = e_r;
        dm.dvz_dx[i] = e_s;
    }
    const float l2m = lam + 2.0f * mu, dl2m = dlam + 2.0f * dmu;
    // propagation term, then the coupling term (the background's source amplitude does not depend on the model), then the source term
    float dszz = (dszz0 + (l2m * E.vz_z + lam * E.vx_x) * g.dt) + (dl2m * D.vz_z + dlam * D.vx_x) * g.dt;
    float dsxx = (dsxx0 + (lam * E.vz_z + l2m * E.vx_x) * g.dt) + (dlam * D.vz_z + dl2m * D.vx_x) * g.dt;
    if constexpr (SRC) {
        if (z == (zx_src >> 16) && x == (zx_src & 0xffff)) {
            dszz += dsrc_amp;
            dsxx += dsrc_amp;
        }
    }
    df.szz[i] = dszz;
    df.sxx[i] = dsxx;
    df.sxz[i] = (dsxz0 + amu * (E.vx_z + E.vz_x) * g.dt) + damu * (D.vx_z + D.vz_x) * g.dt;
}

__global__ __launch_bounds__(MAXT) void k_born_velocity(Grid g, BornArgs b) {
    const Fields f = fields_of(b.state, b.n), df = fields_of(b.dstate, b.n);
    const PmlMem m = b_mem(b.state, b.n), dm = b_mem(b.dstate, b.n);
    const Media md = media_of(b.media, b.n);
    const PmlCoef pc = coef_of(b.cz, b.cz + 6 * g.nzc, g.nzc, g.nx);
    const Cell c = my_cell(g);
    const int z = c.z, x = c.x;
    const size_t i = c.i;
    const bool on = !(z >= g.nzc || x >= g.nx || z < 2 || z > g.nzc - 3 || x < 2 || x > g.nx - 3);  // el_velocity.cu:47
    const bool pz = on && in_pml_z(g, z);
    const bool px = on && (x < g.nPml || x > g.nx - g.nPml);  // el_velocity.cu:56,71 (one column narrower on the right)
    VelD D{}, E{};
    float ba = 0.f, bb = 0.f, dba = 0.f, dbb = 0.f, dvz0 = 0.f, dvx0 = 0.f;
    float e_p = 0.f, e_q = 0.f, e_r = 0.f, e_s = 0.f;
    if (on) {
        D = velocity_derivs(g, f, i);  // the background's stresses after this step's update and source add
        E = velocity_derivs(g, df, i);
        buoyancies(g, md, i, ba, bb);
        dba = b.dmedia[3 * b.n + i];
        dbb = b.dmedia[4 * b.n + i];
        dvz0 = df.vz[i];
        dvx0 = df.vx[i];
        if (pz) {
            const float p = pc.b_zh[z] * m.dszz_dz[i] + pc.a_zh[z] * D.szz_z;
            D.szz_z = D.szz_z * pc.rK_zh[z] + p;
            const float q = pc.b_z[z] * m.dsxz_dz[i] + pc.a_z[z] * D.sxz_z;
            D.sxz_z = D.sxz_z * pc.rK_z[z] + q;
            e_p = pc.b_zh[z] * dm.dszz_dz[i] + pc.a_zh[z] * E.szz_z;
            E.szz_z = E.szz_z * pc.rK_zh[z] + e_p;
            e_q = pc.b_z[z] * dm.dsxz_dz[i] + pc.a_z[z] * E.sxz_z;
            E.sxz_z = E.sxz_z * pc.rK_z[z] + e_q;
        }
        if (px) {
            const float p = pc.b_x[x] * m.dsxz_dx[i] + pc.a_x[x] * D.sxz_x;
            D.sxz_x = D.sxz_x * pc.rK_x[x] + p;
            const float q = pc.b_xh[x] * m.dsxx_dx[i] + pc.a_xh[x] * D.sxx_x;
            D.sxx_x = D.sxx_x * pc.rK_xh[x] + q;
            e_r = pc.b_x[x] * dm.dsxz_dx[i] + pc.a_x[x] * E.sxz_x;
            E.sxz_x = E.sxz_x * pc.rK_x[x] + e_r;
            e_s = pc.b_xh[x] * dm.dsxx_dx[i] + pc.a_xh[x] * E.sxx_x;
            E.sxx_x = E.sxx_x * pc.rK_xh[x] + e_s;
        }
    }
    velocity_body<true>(g, c, f, m, md, pc, nullptr, -1, -1, 0.0f, nullptr, Fields{}, AccG{});
    if (!on) return;
    if (pz) {
        dm.dszz_dz[i] = e_p;
        dm.dsxz_dz[i] = e_q;
    }
    if (px) {
        dm.dsxz_dx[i] = e_r;
        dm.dsxx_dx[i] = e_s;
    }
    df.vz[i] = (dvz0 + (E.szz_z + E.sxz_x) * ba * g.dt) + (D.szz_z + D.sxz_x) * dba * g.dt;
    df.vx[i] = (dvx0 + (E.sxz_z + E.sxx_x) * bb * g.dt) + (D.sxz_z + D.sxx_x) * dbb * g.dt;
}

// perturbed media (born.hpp), in the launch shape of k_model_prep: dense (nz, nx) inputs, pitched outputs on the nzc stored rows.
// The averages of the background are the session's own arrays (what the kernels propagate with).
__global__ void k_born_media(Grid g, const float *__restrict__ Mu_in, const float *__restrict__ dLam_in, const float *__restrict__ dMu_in,
                             const float *__restrict__ dDen_in, Media md, float *__restrict__ dlam, float *__restrict__ dmu, float *__restrict__ damu,
                             float *__restrict__ dba, float *__restrict__ dbb) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int z = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= g.nx || z >= g.nzc) return;
    const size_t si = (size_t)z * g.nx + x, i = (size_t)z * g.pitch + x;
    dlam[i] = (float)((double)dLam_in[si] * 1e6);
    dmu[i] = (float)((double)dMu_in[si] * 1e6);
    float am_d = 0.0f, a_d = 0.0f, b_d = 0.0f;  // outside [2, n-3]^2 the averages are constants (Model.cu:67,72-73)
    if (z >= 2 && z <= g.nz - 3 && x >= 2 && x <= g.nx - 3) {
        const double am = md.ave_mu[i];
        if (am != 0.0) {  // (a zero average: one of the four cells is a fluid, the rule gives 0 whatever the others are)
            double s = 0.0;
            const size_t k4[4] = {si, si + (size_t)g.nx, si + 1, si + (size_t)g.nx + 1};
            for (int k = 0; k < 4; k++) {
                const double m_k = (double)(float)((double)Mu_in[k4[k]] * 1e6);
                s += ((double)dMu_in[k4[k]] * 1e6) / (m_k * m_k);
            }
            am_d = (float)(am * am * 0.25 * s);
        }
        const double ba = md.byc_a[i], bb = md.byc_b[i];
        a_d = (float)(-(ba * ba) * 0.5 * ((double)dDen_in[si + g.nx] + (double)dDen_in[si]));
        b_d = (float)(-(bb * bb) * 0.5 * ((double)dDen_in[si + 1] + (double)dDen_in[si]));
    }
    damu[i] = am_d;
    dba[i] = a_d;
    dbb[i] = b_d;
}

void launch_born_stress(hipStream_t st, const Grid &g0, const KernelOptions &o, const BornArgs &b, float *frame_t, int z_src, int x_src, float src_amp,
                        const float *dsrc_amp) {
    const Grid g = tiled(g0, o, 0);  // the forward kernels' tiling: the background takes the paths of a plain forward pass
    auto k = dsrc_amp ? (frame_t ? k_born_stress<true, true> : k_born_stress<false, true>) : (frame_t ? k_born_stress<true, false> : k_born_stress<false, false>);
    hipLaunchKernelGGL(k, dim3(g.nblk), dim3(BX * g.bz), 0, st, g, b, frame_t, (z_src << 16) | x_src, src_amp, dsrc_amp ? *dsrc_amp : 0.0f);
}

void launch_born_velocity(hipStream_t st, const Grid &g0, const KernelOptions &o, const BornArgs &b) {
    const Grid g = tiled(g0, o, 0);  // the forward kernels' tiling: the background takes the paths of a plain forward pass
    hipLaunchKernelGGL(k_born_velocity, dim3(g.nblk), dim3(BX * g.bz), 0, st, g, b);
}

void launch_born_media(hipStream_t st, const Grid &g, const float *Mu_in, const float *dLam_in, const float *dMu_in, const float *dDen_in, Media md,
                       float *dmedia, size_t n) {
    hipLaunchKernelGGL(k_born_media, dim3((g.nx + 63) / 64, (g.nz + 3) / 4), dim3(64, 4), 0, st, g, Mu_in, dLam_in, dMu_in, dDen_in, md, dmedia,
                       dmedia + n, dmedia + 2 * n, dmedia + 3 * n, dmedia + 4 * n);
}

}  // namespace sepfwi
