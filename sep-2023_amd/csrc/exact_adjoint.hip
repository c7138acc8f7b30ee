// exact_adjoint.hip -- the kernels of the exact discrete adjoint (exact_adjoint.hpp).  A translation unit of its own: the field kernels
// (kernels.hip) are untouched.  Bundle unpacking, region, strip and Omega tests (kernels_device.hpp) and the launch tiling (tiled(),
// kernels.hpp) are the field kernels' own.
//
// k_exact_a / k_exact_b keep the pairing, the launch shape and the cell mapping of k_bwd_a / k_bwd_b (one wave per 64-column row
// segment, my_cell) and call the reverse-time bodies (velocity_body<false>, stress_body<false, false>, kernels_bodies.hpp: the same
// inline code compiled with the same flags) unchanged, so reconstruction, frame restore and the five raw imaging accumulators are those
// of a gradient call.  The two adjoint bodies are new: the exact transposes of stress_body<true> and velocity_body<true>, split into
// LOAD (every tap, issued before the reverse-time body's first store) and APPLY (own-cell stores, adjoint memories) like the bodies
// they stand in for.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "exact_adjoint.hpp"

namespace sepfwi {
#include "kernels_device.hpp"
#include "kernels_bodies.hpp"

namespace {

// What a forward cell (profile index k, flat index j) hands back to the field it differenced: e / K + a P inside its strip, e outside
__device__ __forceinline__ float pml_tap(bool in, float e, const float *__restrict__ rK, const float *__restrict__ a, const float *P, int k, size_t j) {
    return in ? e * rK[k] + a[k] * P[j] : e;
}

// ---------------------------------------------------------------------------------------------
// V^T: adjoint stresses from the adjoint velocities (transpose of velocity_body<true>)
// ---------------------------------------------------------------------------------------------
struct VtIn {
    bool on;
    float szz, sxx, sxz, uz, ux, us;
};
__device__ __forceinline__ VtIn exact_vt_load(const Grid &g, const Cell &c, const Fields &a, const PmlMem &m, const Media &md, const PmlCoef &pc) {
    VtIn q;
    const int z = c.z, x = c.x, P = g.pitch;
    q.on = on_region(g, z, x);
    if (!q.on) return q;
    const size_t i = c.i;
    q.szz = a.szz[i];
    q.sxx = a.sxx[i];
    q.sxz = a.sxz[i];
    auto fz = [&](size_t j) { return md.byc_a[j] * a.vz[j] * g.dt; };
    auto fx = [&](size_t j) { return md.byc_b[j] * a.vx[j] * g.dt; };
    // Only the cells of R are rows of V: a tap outside R hands nothing back.  The adjoint velocities are NOT zero there -- the injection of
    // a channel on the first row or column of R (or, directional, on the last) writes one cell outside it, where nothing ever clears it.
    auto row_on = [&](int zt) { return zt >= 2 && zt <= g.nzc - 3; };
    auto col_on = [&](int xt) { return xt >= 2 && xt <= g.nx - 3; };
    float e1[4], e3[4], e2[4], e4[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        {   // z taps z-2 .. z+1 (D-z) of fz: the forward cell differenced szz with D+z, memory dszz_dz, half profiles
            const int zt = z + k - 2;
            const size_t j = i + (size_t)((long long)(k - 2) * P);
            e1[k] = row_on(zt) ? pml_tap(in_pml_z(g, zt), fz(j), pc.rK_zh, pc.a_zh, m.dszz_dz, zt, j) : 0.0f;
        }
        {   // z taps z-1 .. z+2 (D+z) of fx: sxz differenced with D-z, memory dsxz_dz
            const int zt = z + k - 1;
            const size_t j = i + (size_t)((long long)(k - 1) * P);
            e3[k] = row_on(zt) ? pml_tap(in_pml_z(g, zt), fx(j), pc.rK_z, pc.a_z, m.dsxz_dz, zt, j) : 0.0f;
        }
        {   // x taps x-1 .. x+2 (D+x) of fz: sxz differenced with D-x, memory dsxz_dx
            const int xt = x + k - 1;
            const size_t j = i + k - 1;
            e2[k] = col_on(xt) ? pml_tap(strip_xv(g, xt), fz(j), pc.rK_x, pc.a_x, m.dsxz_dx, xt, j) : 0.0f;
        }
        {   // x taps x-2 .. x+1 (D-x) of fx: sxx differenced with D+x, memory dsxx_dx, half profiles
            const int xt = x + k - 2;
            const size_t j = i + k - 2;
            e4[k] = col_on(xt) ? pml_tap(strip_xv(g, xt), fx(j), pc.rK_xh, pc.a_xh, m.dsxx_dx, xt, j) : 0.0f;
        }
    }
    q.uz = -dminus(e1[0], e1[1], e1[2], e1[3], g.rdz);
    q.ux = -dminus(e4[0], e4[1], e4[2], e4[3], g.rdx);
    q.us = -dplus(e2[0], e2[1], e2[2], e2[3], g.rdx) - dplus(e3[0], e3[1], e3[2], e3[3], g.rdz);
    return q;
}
__device__ __forceinline__ void exact_vt_apply(const VtIn &q, const Grid &g, const Cell &c, const Fields &a, const PmlMem &m, const Media &md,
                                               const PmlCoef &pc) {
    if (!q.on) return;
    const int z = c.z, x = c.x;
    const size_t i = c.i;
    const float szz = q.szz + q.uz, sxx = q.sxx + q.ux, sxz = q.sxz + q.us;
    a.szz[i] = szz;
    a.sxx[i] = sxx;
    a.sxz[i] = sxz;
    const bool pz = in_pml_z(g, z), px = strip_xs(g, x);
    if (pz || px) {  // the adjoint memories of the stress update, on its own strips: P <- b P + e
        const float lam = md.lam[i], l2m = lam + 2.0f * md.mu[i];
        const float e3 = md.ave_mu[i] * sxz * g.dt;
        if (pz) {
            m.dvz_dz[i] = pc.b_z[z] * m.dvz_dz[i] + (l2m * szz + lam * sxx) * g.dt;
            m.dvx_dz[i] = pc.b_zh[z] * m.dvx_dz[i] + e3;
        }
        if (px) {
            m.dvx_dx[i] = pc.b_x[x] * m.dvx_dx[i] + (lam * szz + l2m * sxx) * g.dt;
            m.dvz_dx[i] = pc.b_xh[x] * m.dvz_dx[i] + e3;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// S^T: adjoint velocities from the adjoint stresses (transpose of stress_body<true>)
// ---------------------------------------------------------------------------------------------
struct StIn {
    bool on;
    float vz, vx, uz, ux;
};
__device__ __forceinline__ StIn exact_st_load(const Grid &g, const Cell &c, const Fields &a, const PmlMem &m, const Media &md, const PmlCoef &pc) {
    StIn q;
    const int z = c.z, x = c.x, P = g.pitch;
    q.on = on_region(g, z, x);
    if (!q.on) return q;
    const size_t i = c.i;
    q.vz = a.vz[i];
    q.vx = a.vx[i];
    auto e1 = [&](size_t j) { const float lam = md.lam[j]; return ((lam + 2.0f * md.mu[j]) * a.szz[j] + lam * a.sxx[j]) * g.dt; };
    auto e2 = [&](size_t j) { const float lam = md.lam[j]; return (lam * a.szz[j] + (lam + 2.0f * md.mu[j]) * a.sxx[j]) * g.dt; };
    auto e3 = [&](size_t j) { return md.ave_mu[j] * a.sxz[j] * g.dt; };
    float g1[4], g2[4], g3[4], g4[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        {   // z taps z-1 .. z+2 (D+z) of e1: vz differenced with D-z, memory dvz_dz
            const int zt = z + k - 1;
            const size_t j = i + (size_t)((long long)(k - 1) * P);
            g1[k] = pml_tap(in_pml_z(g, zt), e1(j), pc.rK_z, pc.a_z, m.dvz_dz, zt, j);
        }
        {   // z taps z-2 .. z+1 (D-z) of e3: vx differenced with D+z, memory dvx_dz, half profiles
            const int zt = z + k - 2;
            const size_t j = i + (size_t)((long long)(k - 2) * P);
            g3[k] = pml_tap(in_pml_z(g, zt), e3(j), pc.rK_zh, pc.a_zh, m.dvx_dz, zt, j);
        }
        {   // x taps x-1 .. x+2 (D+x) of e2: vx differenced with D-x, memory dvx_dx
            const int xt = x + k - 1;
            const size_t j = i + k - 1;
            g2[k] = pml_tap(strip_xs(g, xt), e2(j), pc.rK_x, pc.a_x, m.dvx_dx, xt, j);
        }
        {   // x taps x-2 .. x+1 (D-x) of e3: vz differenced with D+x, memory dvz_dx, half profiles
            const int xt = x + k - 2;
            const size_t j = i + k - 2;
            g4[k] = pml_tap(strip_xs(g, xt), e3(j), pc.rK_xh, pc.a_xh, m.dvz_dx, xt, j);
        }
    }
    q.uz = -dplus(g1[0], g1[1], g1[2], g1[3], g.rdz) - dminus(g4[0], g4[1], g4[2], g4[3], g.rdx);
    q.ux = -dplus(g2[0], g2[1], g2[2], g2[3], g.rdx) - dminus(g3[0], g3[1], g3[2], g3[3], g.rdz);
    return q;
}
__device__ __forceinline__ void exact_st_apply(const StIn &q, const Grid &g, const Cell &c, const Fields &a, const PmlMem &m, const Media &md,
                                               const PmlCoef &pc) {
    if (!q.on) return;
    const int z = c.z, x = c.x;
    const size_t i = c.i;
    const float vz = q.vz + q.uz, vx = q.vx + q.ux;
    a.vz[i] = vz;
    a.vx[i] = vx;
    const bool pz = in_pml_z(g, z), px = strip_xv(g, x);
    if (pz || px) {  // the adjoint memories of the velocity update, on its own strips: Q <- b Q + f
        const float fz = md.byc_a[i] * vz * g.dt, fx = md.byc_b[i] * vx * g.dt;
        if (pz) {
            m.dszz_dz[i] = pc.b_zh[z] * m.dszz_dz[i] + fz;
            m.dsxz_dz[i] = pc.b_z[z] * m.dsxz_dz[i] + fx;
        }
        if (px) {
            m.dsxz_dx[i] = pc.b_x[x] * m.dsxz_dx[i] + fz;
            m.dsxx_dx[i] = pc.b_xh[x] * m.dsxx_dx[i] + fx;
        }
    }
}

}  // namespace

__global__ __launch_bounds__(MAXT) void k_exact_a(Grid g, ExactArgs b, const float *__restrict__ frame_t) {
    const Fields f = fields_of(b.fields, b.n), adj = fields_of(b.adj, b.n);
    const PmlMem m = mem_of(b.mem, b.n);
    const Media md = media_of(b.media, b.n);
    const ImgAcc acc = acc_of(b.acc, b.n);
    const PmlCoef pc = coef_of(b.cz, b.cz + 6 * g.nzc, g.nzc, g.nx);
    const Cell c = my_cell(g);
    const VtIn q = exact_vt_load(g, c, adj, m, md, pc);  // (in flight together with the reverse-velocity loads)
    velocity_body<false>(g, c, f, m, md, pc, frame_t, -1, -1, 0.0f, nullptr, adj, AccG{acc});
    exact_vt_apply(q, g, c, adj, m, md, pc);
}

// SRC: the transpose of the source add, a gather -- the lane that owns the source cell stores s_zz + s_xx of the adjoint stresses as they
// stand between V^T and S^T of this step (this kernel reads them through its taps and never writes them) to g_amp_it.  They are loaded
// with the taps, before the reverse-time body's first store, and stored after the last one: a store keeps later may-alias loads behind
// it.  The instance without the gather is the kernel as it always was.
template <bool SRC>
__global__ __launch_bounds__(MAXT) void k_exact_b(Grid g, ExactArgs b, float *__restrict__ frame_t, int zx_src /* z<<16 | x */, float src_amp,
                                                  int adjoint_only, float *__restrict__ g_amp_it) {
    const Fields f = fields_of(b.fields, b.n), adj = fields_of(b.adj, b.n);
    const PmlMem m = mem_of(b.mem, b.n);
    const Media md = media_of(b.media, b.n);
    const ImgAcc acc = acc_of(b.acc, b.n);
    const PmlCoef pc = coef_of(b.cz, b.cz + 6 * g.nzc, g.nzc, g.nx);
    const Cell c = my_cell(g);
    const StIn q = exact_st_load(g, c, adj, m, md, pc);
    bool at_src = false;
    float g_amp = 0.0f;
    if constexpr (SRC) {
        at_src = c.z == (zx_src >> 16) && c.x == (zx_src & 0xffff);
        if (at_src) g_amp = adj.szz[c.i] + adj.sxx[c.i];
    }
    if (!adjoint_only)  // launch-uniform
        stress_body<false, false>(g, c, f, m, md, pc, frame_t, zx_src >> 16, zx_src & 0xffff, src_amp, adj, AccG{acc}, LineRec{});
    exact_st_apply(q, g, c, adj, m, md, pc);
    if constexpr (SRC) {
        if (at_src) *g_amp_it = g_amp;
    }
}

// The transposes of k_born_media's maps on Omega (exact_adjoint.hpp), in the launch shape of k_finalize_gradients: dense (nz, nx) outputs.
__global__ void k_exact_finalize(Grid g, Media md, ImgAcc acc, float *__restrict__ gLam, float *__restrict__ gMu, float *__restrict__ gDen) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int z = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= g.nx || z >= g.nz) return;
    const size_t o = (size_t)z * g.nx + x;
    float gl = 0.0f, gm = 0.0f, gd = 0.0f;
    if (in_omega(g, z, x)) {
        const size_t i = (size_t)z * g.pitch + x, P = (size_t)g.pitch;
        gl = (float)((double)acc.lam[i] * 1e6);
        const double mu = md.mu[i];
        double s = 0.0;
        const size_t p4[4] = {i, i - P, i - 1, i - P - 1};  // the four staggered corners whose harmonic mean holds this cell
        for (int k = 0; k < 4; k++) {
            const double am = md.ave_mu[p4[k]];
            if (am != 0.0) s += am * am * 0.25 * (double)acc.xz[p4[k]];  // (a zero average: a fluid corner, its derivative is 0)
        }
        gm = (float)(((double)acc.mu[i] + (mu != 0.0 ? s / (mu * mu) : 0.0)) * 1e6);
        const double a0 = md.byc_a[i], a1 = md.byc_a[i - P], b0 = md.byc_b[i], b1 = md.byc_b[i - 1];
        gd = (float)(-0.5 * (a0 * a0 * (double)acc.a[i] + a1 * a1 * (double)acc.a[i - P] + b0 * b0 * (double)acc.b[i] + b1 * b1 * (double)acc.b[i - 1]));
    }
    gLam[o] = gl;
    gMu[o] = gm;
    gDen[o] = gd;
}

__global__ void k_exact_mask(Grid g, float *__restrict__ v, int k, size_t dense) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int z = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= g.nx || z >= g.nz) return;
    if (in_omega(g, z, x)) return;
    for (int a = 0; a < k; a++) v[(size_t)a * dense + (size_t)z * g.nx + x] = 0.0f;
}

void launch_exact_a(hipStream_t st, const Grid &g0, const KernelOptions &o, const ExactArgs &b, const float *frame_t) {
    const Grid g = tiled(g0, o, 1);  // the backward kernels' tiling: the reverse-time bodies take the paths of a gradient call
    hipLaunchKernelGGL(k_exact_a, dim3(g.nblk), dim3(BX * g.bz), 0, st, g, b, frame_t);
}

void launch_exact_b(hipStream_t st, const Grid &g0, const KernelOptions &o, const ExactArgs &b, float *frame_t, int z_src, int x_src, float src_amp,
                    bool adjoint_only, float *g_amp_it) {
    const Grid g = tiled(g0, o, 1);  // the backward kernels' tiling: the reverse-time bodies take the paths of a gradient call
    const int zx = adjoint_only ? 0 : (z_src << 16) | x_src;
    if (adjoint_only) g_amp_it = nullptr;  // (no amplitude follows the last velocity update: the priming launch gathers nothing)
    auto k = g_amp_it ? k_exact_b<true> : k_exact_b<false>;
    hipLaunchKernelGGL(k, dim3(g.nblk), dim3(BX * g.bz), 0, st, g, b, frame_t, zx, src_amp, adjoint_only ? 1 : 0, g_amp_it);
}

void launch_exact_finalize(hipStream_t st, const Grid &g, Media md, ImgAcc acc, float *gLam, float *gMu, float *gDen) {
    hipLaunchKernelGGL(k_exact_finalize, dim3((g.nx + 63) / 64, (g.nz + 3) / 4), dim3(64, 4), 0, st, g, md, acc, gLam, gMu, gDen);
}

void launch_exact_mask(hipStream_t st, const Grid &g, float *v, int k, size_t dense) {
    hipLaunchKernelGGL(k_exact_mask, dim3((g.nx + 63) / 64, (g.nz + 3) / 4), dim3(64, 4), 0, st, g, v, k, dense);
}

}  // namespace sepfwi
