// pseudo_hessian.hip -- the kernels of the diagonal pseudo-Hessian (pseudo_hessian.hpp).  A translation unit of its own: the field
// kernels (kernels.hip) are untouched.
//
// Structure of the two accumulating kernels: one wave per 64-column row segment of the grid that meets the interior, x fastest, as the
// field kernels walk the grid (lanes outside the interior leave at once).  Every neighbour tap is a shifted global load -- no LDS halo,
// no cross-lane shuffle (profiles/r04_xtap_probe.txt: 5-24 % slower on this chip) -- and every load of a cell is issued before its
// first store.  The accumulators are read and written with plain vector loads / stores: each cell belongs to one lane
// of one wave of one launch, and the launches that share a set are ordered by their stream, so there is no atomic anywhere and the
// sums are reproducible bit for bit.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "pseudo_hessian.hpp"

namespace sepfwi {

using dev::dminus;
using dev::dplus;

// the three terms of one shot at interior cell i (pseudo_hessian.hpp); P = pitch, ba / bb the buoyancies of index i
__device__ __forceinline__ void ph_terms(const float *__restrict__ vz, const float *__restrict__ vx, const float *__restrict__ szz,
                                         const float *__restrict__ sxx, const float *__restrict__ sxz, size_t i, int P, float rdz, float rdx,
                                         float ba, float bb, float &t_lam, float &t_mu, float &t_rho) {
    const float vz0 = vz[i], vx0 = vx[i], sxz0 = sxz[i];
    const float a = dminus(vz[i - 2 * P], vz[i - P], vz0, vz[i + P], rdz);                     // dvz_dz
    const float b = dminus(vx[i - 2], vx[i - 1], vx0, vx[i + 1], rdx);                         // dvx_dx
    const float dvx_dz = dplus(vx[i - P], vx0, vx[i + P], vx[i + 2 * P], rdz);
    const float dvz_dx = dplus(vz[i - 1], vz0, vz[i + 1], vz[i + 2], rdx);
    const float dszz_dz = dplus(szz[i - P], szz[i], szz[i + P], szz[i + 2 * P], rdz);
    const float dsxz_dx = dminus(sxz[i - 2], sxz[i - 1], sxz0, sxz[i + 1], rdx);
    const float dsxz_dz = dminus(sxz[i - 2 * P], sxz[i - P], sxz0, sxz[i + P], rdz);
    const float dsxx_dx = dplus(sxx[i - 1], sxx[i], sxx[i + 1], sxx[i + 2], rdx);
    const float s = dvx_dz + dvz_dx, ab = a + b;
    const float fz = ba * ba * 0.5f * (dszz_dz + dsxz_dx), fx = bb * bb * 0.5f * (dsxz_dz + dsxx_dx);
    t_lam = ab * ab;
    t_mu = 4.0f * a * a + 4.0f * b * b + s * s;
    t_rho = fz * fz + fx * fx;
}

// Interior cell of this lane: wave w of the launch owns row nPml + w / nseg, row segment seg0 + w % nseg.  False: nothing to do.
__device__ __forceinline__ bool ph_cell(const Grid &g, int seg0, int nseg, size_t &i) {
    const int w = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    const int z = g.nPml + w / nseg, x = ((seg0 + w % nseg) << 6) + lane;
    if (z > g.zmax || x < g.nPml || x > g.xmax) return false;
    i = (size_t)z * (size_t)g.pitch + (size_t)x;
    return true;
}

__global__ __launch_bounds__(256) void k_pseudo_hessian(Grid g, Fields f, const float *__restrict__ rho, PhAcc acc, float weight, int seg0, int nseg) {
    size_t i;
    if (!ph_cell(g, seg0, nseg, i)) return;
    const float r0 = rho[i], ba = 2.0f / (rho[i + g.pitch] + r0), bb = 2.0f / (rho[i + 1] + r0);  // buoyancies(), kernels_bodies.hpp
    const float e_lam = acc.lam[i], e_mu = acc.mu[i], e_rho = acc.rho[i];
    float t_lam, t_mu, t_rho;
    ph_terms(f.vz, f.vx, f.szz, f.sxx, f.sxz, i, g.pitch, g.rdz, g.rdx, ba, bb, t_lam, t_mu, t_rho);
    acc.lam[i] = e_lam + weight * t_lam;
    acc.mu[i] = e_mu + weight * t_mu;
    acc.rho[i] = e_rho + weight * t_rho;
}

// batched twin: the wave loops over the shots of the sub-batch in table order (ShotDev::fields: vz, vx, szz, sxx, sxz at stride n) and
// does ONE read-modify-write of the accumulators -- a fixed order of the adds, and the accumulator traffic is shared by the batch
__global__ __launch_bounds__(256) void k_pseudo_hessian_batch(Grid g, const ShotDev *__restrict__ shots, int nb, size_t n,
                                                               const float *__restrict__ rho, PhAcc acc, float weight, int seg0, int nseg) {
    size_t i;
    if (!ph_cell(g, seg0, nseg, i)) return;
    const float r0 = rho[i], ba = 2.0f / (rho[i + g.pitch] + r0), bb = 2.0f / (rho[i + 1] + r0);
    float e_lam = acc.lam[i], e_mu = acc.mu[i], e_rho = acc.rho[i];
    for (int k = 0; k < nb; k++) {
        const float *__restrict__ b = shots[k].fields;
        float t_lam, t_mu, t_rho;
        ph_terms(b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, i, g.pitch, g.rdz, g.rdx, ba, bb, t_lam, t_mu, t_rho);
        e_lam = e_lam + weight * t_lam;
        e_mu = e_mu + weight * t_mu;
        e_rho = e_rho + weight * t_rho;
    }
    acc.lam[i] = e_lam;
    acc.mu[i] = e_mu;
    acc.rho[i] = e_rho;
}

// the sets summed in index order in double, the constants of pseudo_hessian.hpp applied; dense (nz, nx), zero outside the interior
__global__ void k_pseudo_hessian_finalize(Grid g, PhSets sets, size_t n, double c_lam, double c_mu, double c_rho, float *__restrict__ hLam,
                                          float *__restrict__ hMu, float *__restrict__ hDen) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int z = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= g.nx || z >= g.nz) return;
    const size_t o = (size_t)z * g.nx + x;
    double e_lam = 0.0, e_mu = 0.0, e_rho = 0.0;
    if (z >= g.nPml && z <= g.zmax && x >= g.nPml && x <= g.xmax) {
        const size_t i = (size_t)z * g.pitch + x;
        for (int k = 0; k < sets.nsets; k++) {
            e_lam += (double)sets.set[k][i];
            e_mu += (double)sets.set[k][n + i];
            e_rho += (double)sets.set[k][2 * n + i];
        }
    }
    hLam[o] = (float)(c_lam * e_lam);
    hMu[o] = (float)(c_mu * e_mu);
    hDen[o] = (float)(c_rho * e_rho);
}

// waves of an accumulating launch: interior rows x row segments of the grid that meet the interior columns
static bool ph_geometry(const Grid &g, int &seg0, int &nseg, int &blocks) {
    const int rows = g.zmax - g.nPml + 1;
    if (rows <= 0 || g.xmax < g.nPml) return false;
    seg0 = g.nPml >> 6;
    nseg = (g.xmax >> 6) - seg0 + 1;
    blocks = (rows * nseg + 3) / 4;  // 4 waves per block
    return true;
}

void launch_pseudo_hessian(hipStream_t st, const Grid &g, Fields f, Media md, PhAcc acc, float weight) {
    int seg0, nseg, blocks;
    if (!ph_geometry(g, seg0, nseg, blocks)) return;
    hipLaunchKernelGGL(k_pseudo_hessian, dim3(blocks), dim3(256), 0, st, g, f, md.rho, acc, weight, seg0, nseg);
}

void launch_pseudo_hessian_batch(hipStream_t st, const Grid &g, const ShotDev *shots, int nb, size_t n, Media md, PhAcc acc, float weight) {
    int seg0, nseg, blocks;
    if (nb <= 0 || !ph_geometry(g, seg0, nseg, blocks)) return;
    hipLaunchKernelGGL(k_pseudo_hessian_batch, dim3(blocks), dim3(256), 0, st, g, shots, nb, n, md.rho, acc, weight, seg0, nseg);
}

void launch_pseudo_hessian_finalize(hipStream_t st, const Grid &g, PhSets sets, size_t n, double c_lam, double c_mu, double c_rho, float *hLam,
                                    float *hMu, float *hDen) {
    const dim3 blk(64, 4), grd((g.nx + 63) / 64, (g.nz + 3) / 4);
    hipLaunchKernelGGL(k_pseudo_hessian_finalize, grd, blk, 0, st, g, sets, n, c_lam, c_mu, c_rho, hLam, hMu, hDen);
}

}  // namespace sepfwi
