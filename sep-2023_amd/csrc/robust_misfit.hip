// robust_misfit.hip -- the kernel of the robust misfits (robust_misfit.hpp holds the definition).
//
// One workgroup of 256 threads (four waves) per trace, in two phases:
//   1  A: an exact radix select on the bit patterns of |o_i|, i = 1 ... nt - 1.  Non-negative float32 values order like their unsigned
//      bits; the sign bit is cleared, so -0 counts as +0.  Four passes of 8 bits from the top: every pass counts the samples that still
//      match the digits found so far into a 256-bin histogram in LDS (integer LDS atomics: the counts do not depend on their order), one
//      thread per bin takes the inclusive scan of the counts (64-lane shuffles, the four wave totals through LDS), and the one bin whose
//      range of ranks holds k becomes the next digit; k is reduced by the count below it.  After the fourth pass the digits ARE the bits of
//      the order statistic -- exact for ties, constant traces, k = 0 and k = n - 1, because equal values fall into the same bin in every
//      pass and the scan counts them all.
//   2  the pointwise pass in double: psi and 2 sum phi (a block reduction in a fixed order), or the product sign Z w Z d.
// The trace (16 KB at 4000 samples) is read five times by the block that owns it: once from HBM, then from cache.
#include <hip/hip_runtime.h>

#include <cmath>

#include "robust_misfit.hpp"

namespace sepfwi {

namespace {

constexpr int kBlock = 256;

struct RobustLds {
    unsigned hist[kBlock];  // the counts of a pass, one bin per thread
    unsigned wave[4];       // the wave totals of its scan
    unsigned digit, below;  // the bin that holds rank k, and the count of the bins under it
    double red[4];          // the wave partials of the reduction
};

// the bits of the rank-th smallest (from 0) of |o[1]| ... |o[nt - 1]|; 0 <= rank < nt - 1.  Called by ALL threads; the same value in each.
__device__ __forceinline__ unsigned select_abs_bits(const float *__restrict__ o, int nt, unsigned rank, RobustLds &lds) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        lds.hist[tid] = 0;
        __syncthreads();
        for (int i = 1 + tid; i < nt; i += kBlock) {
            const unsigned b = __float_as_uint(o[i]) & 0x7fffffffu;
            if ((b & mask) == prefix) atomicAdd(&lds.hist[(b >> shift) & 255u], 1u);
        }
        __syncthreads();
        const unsigned c = lds.hist[tid];
        unsigned incl = c;
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) lds.wave[w] = incl;
        __syncthreads();
        for (int k = 0; k < w; k++) incl += lds.wave[k];
        const unsigned excl = incl - c;
        if (c > 0 && excl <= rank && rank < incl) {  // exactly one bin: the counts sum to more than rank
            lds.digit = (unsigned)tid;
            lds.below = excl;
        }
        __syncthreads();
        prefix |= lds.digit << shift;
        mask |= 255u << shift;
        rank -= lds.below;
    }
    return prefix;
}

__global__ __launch_bounds__(kBlock) void k_robust_trace(int nt, const float *__restrict__ obs, const float *__restrict__ syn,
                                                         const float *__restrict__ d, float *__restrict__ res, int kind, double delta_rel, int rank,
                                                         float sign, float *__restrict__ scale, double *__restrict__ sum) {
    __shared__ RobustLds lds;
    const int r = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)r * nt;
    const float *o = obs + row, *s = syn + row, *dd = d ? d + row : nullptr;
    float *a = res + row;

    const float A = nt >= 2 ? __uint_as_float(select_abs_bits(o, nt, (unsigned)rank, lds)) : 0.0f;
    if (tid == 0) scale[r] = A;
    if (!(A > 0.0f)) {  // a dead trace (the whole block takes the branch)
        for (int i = tid; i < nt; i += kBlock) a[i] = 0.0f;
        if (tid == 0 && !dd) sum[r] = 0.0;
        return;
    }
    const double delta = delta_rel * (double)A, d2 = delta * delta;
    double part = 0.0;
    for (int i = tid; i < nt; i += kBlock) {
        if (i == 0) {
            a[0] = 0.0f;
            continue;
        }
        const double rr = (double)o[i] - (double)s[i], u = rr / delta, au = fabs(u);
        double w, psi, phi;
        if (kind == kRobustHuber) {
            const bool in = au <= 1.0;
            w = in ? 1.0 : 1.0 / au;
            psi = in ? rr : copysign(delta, rr);
            phi = in ? d2 * (0.5 * u * u) : d2 * (au - 0.5);
        } else {
            w = 1.0 / (1.0 + u * u);
            psi = rr * w;
            phi = 0.5 * d2 * log1p(u * u);
        }
        if (dd) {
            a[i] = (float)((double)sign * w * (double)dd[i]);
        } else {
            a[i] = (float)psi;
            part += phi;
        }
    }
    if (dd) return;
    // the block sum in a fixed order: the shuffle tree per wave, then part 0 + 1 + 2 + 3
    for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
    if ((tid & 63) == 0) lds.red[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) sum[r] = 2.0 * (lds.red[0] + lds.red[1] + lds.red[2] + lds.red[3]);
}

}  // namespace

int robust_rank(int nt, double quantile) {
    const int n = nt - 1;
    if (n <= 0) return 0;
    const int k = (int)std::floor(quantile * (double)(n - 1));
    return k < 0 ? 0 : (k > n - 1 ? n - 1 : k);
}

void launch_robust_trace(hipStream_t st, int nt, int nrec, const float *obs, const float *syn, const float *d, float *res, int kind, double delta,
                         int rank, float sign, float *scale, double *sum) {
    hipLaunchKernelGGL(k_robust_trace, dim3(nrec), dim3(kBlock), 0, st, nt, obs, syn, d, res, kind, delta, rank, sign, scale, sum);
}

}  // namespace sepfwi
