// das_gauge.hip -- receivers with a gauge length (das_gauge.hpp): the recording and the adjoint-source injection of gauge channels,
// per shot and batched (blockIdx.y = shot of the batch, side table GaugeShotDev next to the ShotDev table).  A translation unit of its
// own: the field kernels (kernels.hip) are untouched, the persistent loop takes gauge channels through its general-receiver plan.
#include <hip/hip_runtime.h>

#include "das_gauge.hpp"
#include "kernels.hpp"

namespace sepfwi {

// pr / vx / vz at the channel's own cell exactly as record_one (kernels_aux.hpp); ett = the channel's taps summed in tap order
__device__ __forceinline__ void record_gauge_one(const Fields &f, int r, int i, const int *__restrict__ tap_start, const int *__restrict__ tap_cell,
                                                 const int *__restrict__ tap_field, const float *__restrict__ tap_w, float *d_pr, float *d_vx,
                                                 float *d_vz, float *d_ett, int comps) {
    if (comps & 1) d_pr[r] = f.szz[i] + f.sxx[i];
    if (comps & 2) d_vx[r] = f.vx[i];
    if (comps & 4) d_vz[r] = f.vz[i];
    if (!(comps & 8)) return;
    float s = 0.0f;
    for (int e = tap_start[r], e1 = tap_start[r + 1]; e < e1; e++) s += tap_w[e] * (tap_field[e] ? f.vz : f.vx)[tap_cell[e]];
    d_ett[r] = s;
}

// adj[cell of target t] += sum over its entries of w res_t[rec] in entry order -- the loop of k_inject_values (kernels_aux.hpp) and the
// persistent loop's one add per target and step, so every schedule leaves the same bits.  Targets are distinct: no atomics.
__device__ __forceinline__ void inject_gauge_one(float *avz, float *avx, int t, const float *__restrict__ res_t, const int *__restrict__ tgt_start,
                                                 const int *__restrict__ tgt_cell, const int *__restrict__ tgt_field, const int *__restrict__ ent_rec,
                                                 const float *__restrict__ ent_w) {
    const int e0 = tgt_start[t], e1 = tgt_start[t + 1];
    float s = 0.0f;
    for (int e = e0; e < e1; e++) s += ent_w[e] * res_t[ent_rec[e]];
    float *p = (tgt_field[t] ? avz : avx) + tgt_cell[t];
    *p += s;
}

__global__ void k_record_gauge(Fields f, int nrec, const int *__restrict__ rec, const int *__restrict__ tap_start, const int *__restrict__ tap_cell,
                               const int *__restrict__ tap_field, const float *__restrict__ tap_w, float *__restrict__ d_pr, float *__restrict__ d_vx,
                               float *__restrict__ d_vz, float *__restrict__ d_ett, int comps) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrec) return;
    record_gauge_one(f, r, rec[r], tap_start, tap_cell, tap_field, tap_w, d_pr, d_vx, d_vz, d_ett, comps);
}

__global__ void k_inject_gauge(Fields adj, int ntgt, const float *__restrict__ res_t, const int *__restrict__ tgt_start, const int *__restrict__ tgt_cell,
                               const int *__restrict__ tgt_field, const int *__restrict__ ent_rec, const float *__restrict__ ent_w) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntgt) return;
    inject_gauge_one(adj.vz, adj.vx, t, res_t, tgt_start, tgt_cell, tgt_field, ent_rec, ent_w);
}

// batched twins: the shot's arrays from its ShotDev entry (fields, seismograms, adjoint fields, residual), its channels from the side
// table; shots without gauge channels have nrec == ntgt == 0 there
__global__ void k_record_gauge_batch(const ShotDev *__restrict__ shots, const GaugeShotDev *__restrict__ gs, size_t n, size_t data_len, int column) {
    const GaugeShotDev &q = gs[blockIdx.y];
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= q.nrec) return;
    const ShotDev &s = shots[blockIdx.y];
    const Fields f{s.fields, s.fields + n, s.fields + 2 * n, s.fields + 3 * n, s.fields + 4 * n};
    float *col = s.syn + (size_t)column * (size_t)q.nrec;
    record_gauge_one(f, r, q.rec[r], q.tap_start, q.tap_cell, q.tap_field, q.tap_w, col, col + data_len, col + 2 * data_len, col + 3 * data_len, q.comps);
}

__global__ void k_inject_gauge_batch(const ShotDev *__restrict__ shots, const GaugeShotDev *__restrict__ gs, size_t n, int it) {
    const GaugeShotDev &q = gs[blockIdx.y];
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= q.ntgt) return;
    const ShotDev &s = shots[blockIdx.y];
    inject_gauge_one(s.adj, s.adj + n, t, s.res + (size_t)it * (size_t)q.nres, q.tgt_start, q.tgt_cell, q.tgt_field, q.ent_rec, q.ent_w);
}

void launch_record_gauge(hipStream_t st, Fields f, int nrec, const int *rec, const int *tap_start, const int *tap_cell, const int *tap_field,
                         const float *tap_w, float *d_pr, float *d_vx, float *d_vz, float *d_ett, int comps) {
    if (nrec <= 0) return;
    hipLaunchKernelGGL(k_record_gauge, dim3((nrec + 255) / 256), dim3(256), 0, st, f, nrec, rec, tap_start, tap_cell, tap_field, tap_w, d_pr, d_vx, d_vz,
                       d_ett, comps);
}

void launch_inject_gauge(hipStream_t st, Fields adj, int ntgt, const float *res_t, const int *tgt_start, const int *tgt_cell, const int *tgt_field,
                         const int *ent_rec, const float *ent_w) {
    if (ntgt <= 0) return;
    hipLaunchKernelGGL(k_inject_gauge, dim3((ntgt + 255) / 256), dim3(256), 0, st, adj, ntgt, res_t, tgt_start, tgt_cell, tgt_field, ent_rec, ent_w);
}

void launch_record_gauge_batch(hipStream_t st, const ShotDev *shots, const GaugeShotDev *gs, int nb, int max_nrec, size_t n, size_t data_len, int column) {
    if (nb <= 0 || max_nrec <= 0) return;
    hipLaunchKernelGGL(k_record_gauge_batch, dim3((max_nrec + 255) / 256, nb), dim3(256), 0, st, shots, gs, n, data_len, column);
}

void launch_inject_gauge_batch(hipStream_t st, const ShotDev *shots, const GaugeShotDev *gs, int nb, int max_ntgt, size_t n, int it) {
    if (nb <= 0 || max_ntgt <= 0) return;
    hipLaunchKernelGGL(k_inject_gauge_batch, dim3((max_ntgt + 255) / 256, nb), dim3(256), 0, st, shots, gs, n, it);
}

}  // namespace sepfwi
