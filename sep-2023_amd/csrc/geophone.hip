// geophone.hip -- the residual of a joint DAS + geophone misfit (geophone.hpp): one launch per shot (or per batch of shots) turns the
// time-major gathers of the active components into ONE adjoint-source array [it][C nrec], multiplied by the components' weights, and
// forms sum r_c^2 per component in double.  A translation unit of its own: the field kernels (kernels.hip) are untouched; the
// injection of the array goes through the plan kernels that gauge channels use (k_inject_values in the persistent loop,
// k_inject_gauge and its batched twin in the per-step schedules).  k_adjoint_source fills the same array for the passes whose adjoint
// source is not a residual against observed data (Born's J v, the exact adjoint's w).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "geophone.hpp"
#include "kernels.hpp"

namespace sepfwi {

// Column block b of one shot.  r = obs - syn with the first time sample zeroed (gpuMinus, utilities.cu:154-167), k_residual's
// expression; the sum as there: wave shuffle, LDS, one double atomic per block and component.  The launch is a grid-stride loop over
// gridDim.x blocks of 256 threads.
__device__ __forceinline__ void geo_residual_block(const GeoResShot &q, int b, int nSteps, double *__restrict__ sums) {
    const float *__restrict__ obs = q.obs[b], *__restrict__ syn = q.syn[b];
    float *__restrict__ res = q.res + (size_t)b * (size_t)q.nrec;
    const float w = q.w[b];
    const int nrec = q.nrec;
    const size_t row = (size_t)q.nblk * (size_t)nrec;
    const long long n = (long long)nrec * (long long)nSteps;
    double s = 0.0;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
        const long long it = k / nrec;
        const int r = (int)(k - it * nrec);
        const float d = (it == 0) ? 0.0f : (obs[k] - syn[k]);
        res[(size_t)it * row + r] = w * d;
        s += (double)d * (double)d;
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    __shared__ double part[16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) part[wv] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < (int)(blockDim.x >> 6); k++) t += part[k];
        atomicAdd(sums + q.slot[b], t);
    }
}

__global__ void k_geo_residual(GeoResShot q, int nSteps, double *__restrict__ sums) {
    geo_residual_block(q, blockIdx.y, nSteps, sums);  // gridDim.y = q.nblk
}

// batched twin: blockIdx.z = shot of the batch (a shot without channels, or with fewer blocks than the grid has, leaves at once --
// uniformly per block, before the barrier)
__global__ void k_geo_residual_batch(const GeoResShot *__restrict__ shots, int nSteps, double *__restrict__ sums) {
    const GeoResShot &q = shots[blockIdx.z];
    if (q.nrec <= 0 || (int)blockIdx.y >= q.nblk) return;
    geo_residual_block(q, blockIdx.y, nSteps, sums);
}

// The adjoint source from something that is not observed data (AdjSource, geophone.hpp): the same loop over the same layout.
__global__ void k_adjoint_source(AdjSource q, int nSteps) {
    const int b = blockIdx.y;  // gridDim.y = q.nblk
    const float *__restrict__ src = q.src[b];
    float *__restrict__ res = q.res + (size_t)b * (size_t)q.nrec;
    const float scale = q.scale[b];
    const int nrec = q.nrec;
    const size_t row = (size_t)q.nblk * (size_t)nrec;
    const long long n = (long long)nrec * (long long)nSteps;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
        const long long it = k / nrec;
        const int r = (int)(k - it * nrec);
        res[(size_t)it * row + r] = (it == 0 || !src) ? 0.0f : -(scale * src[(size_t)r * q.sr + (size_t)it * q.st]);
    }
}

static int geo_blocks_x(long long n) { return (int)std::min<long long>(1024, std::max<long long>(1, (n + 255) / 256)); }

void launch_geo_residual(hipStream_t st, const GeoResShot &q, int nSteps, double *sums) {
    if (q.nrec <= 0 || q.nblk <= 0) return;
    hipLaunchKernelGGL(k_geo_residual, dim3(geo_blocks_x((long long)q.nrec * nSteps), q.nblk), dim3(256), 0, st, q, nSteps, sums);
}

void launch_adjoint_source(hipStream_t st, const AdjSource &q, int nSteps) {
    if (q.nrec <= 0 || q.nblk <= 0) return;
    hipLaunchKernelGGL(k_adjoint_source, dim3(geo_blocks_x((long long)q.nrec * nSteps), q.nblk), dim3(256), 0, st, q, nSteps);
}

void launch_geo_residual_batch(hipStream_t st, const GeoResShot *shots, int nb, int max_nrec, int max_nblk, int nSteps, double *sums) {
    if (nb <= 0 || max_nrec <= 0 || max_nblk <= 0) return;
    hipLaunchKernelGGL(k_geo_residual_batch, dim3(geo_blocks_x((long long)max_nrec * nSteps), max_nblk, nb), dim3(256), 0, st, shots, nSteps, sums);
}

}  // namespace sepfwi
