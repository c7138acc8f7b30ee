// w2_misfit.hip -- the kernel of the trace-wise quadratic Wasserstein misfit (w2_misfit.hpp holds the definition).
//
// One workgroup of 256 threads (four waves) per trace; the trace is walked in tiles of 256 samples, one sample per thread and tile:
//   1  A = max |o| (block maximum); q(s), q(o) and their inclusive prefix sums: per tile a block scan -- every wave scans its 64 values by
//      shuffles, the four wave totals go through LDS, one carry runs from tile to tile -- then each thread divides its own entries by the
//      totals (the last node of F and of G is x / x = 1)
//   2  per sample the lower bound j(i) over the trace's G (a binary search, its probes served from L2), T_i, (t_i - T_i)^2 and c_i;
//      W as a block sum
//   3  psi: the suffix sums of c are the same block scan on the tiles walked from the trace's END with the threads in reversed order
//      (thread 0 takes the last sample), so that a prefix in thread order is a suffix in time; sum f psi as a block sum
//   4  res, rounded once
// F, G, q(o), q(s) and c live in global scratch (160 KB per trace at 4000 samples: they stay in L2 while the trace's block runs).  A thread
// only ever reads back its OWN entries of F and q(s) inside a phase; G, q(o) and c are read across threads after a barrier
// (__syncthreads orders the block's global writes).  Every sum has a fixed order: the same input gives the same bits.
#include <hip/hip_runtime.h>

#include "w2_misfit.hpp"

namespace sepfwi {

namespace {

constexpr int kTile = 256;

struct W2Lds {
    double wave[2][4];  // the wave totals of a scan round, two scans side by side
    double red[4];      // the wave partials of a reduction
};

__device__ __forceinline__ double softplus(double z) { return fmax(z, 0.0) + log1p(exp(-fabs(z))); }
__device__ __forceinline__ double sigmoid(double z) {
    const double e = exp(-fabs(z));
    return z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

// Inclusive scan of v[n] over the block's 256 threads in thread order, N scans side by side; tot[n]: the block's total, the same bits in
// every thread (and the bits of the last thread's v[n]).  Called by ALL threads of the block.
template <int N> __device__ __forceinline__ void block_scan(double (&v)[N], double (&tot)[N], W2Lds &lds) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int n = 0; n < N; n++)
        for (int off = 1; off < 64; off <<= 1) {
            const double up = __shfl_up(v[n], off, 64);
            if (lane >= off) v[n] += up;
        }
    __syncthreads();  // the round before has read its wave totals
    if (lane == 63)
        for (int n = 0; n < N; n++) lds.wave[n][w] = v[n];
    __syncthreads();
    for (int n = 0; n < N; n++) {
        double before = 0.0, all = 0.0;
        for (int k = 0; k < 4; k++) {
            if (k == w) before = all;
            all += lds.wave[n][k];
        }
        if (w > 0) v[n] = before + v[n];
        tot[n] = all;
    }
}

// Sum (or maximum) of v over the block, the same bits in every thread: the shuffle tree per wave, then part 0 + 1 + 2 + 3 in that order
template <bool MAX> __device__ __forceinline__ double block_all(double v, W2Lds &lds) {
    for (int off = 32; off > 0; off >>= 1) {
        const double other = __shfl_down(v, off, 64);
        v = MAX ? fmax(v, other) : v + other;
    }
    __syncthreads();  // the reduction before has read its partials
    if ((threadIdx.x & 63) == 0) lds.red[threadIdx.x >> 6] = v;
    __syncthreads();
    return MAX ? fmax(fmax(lds.red[0], lds.red[1]), fmax(lds.red[2], lds.red[3])) : lds.red[0] + lds.red[1] + lds.red[2] + lds.red[3];
}

__global__ __launch_bounds__(kTile) void k_w2_trace(int nt, const float *__restrict__ obs, const float *__restrict__ syn, float *__restrict__ res,
                                                    const float *__restrict__ weights, float src_weight, float dt_f, double beta, double *scratch,
                                                    size_t plane, double *__restrict__ wsum) {
    __shared__ W2Lds lds;
    const int r = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)r * nt;
    const float *o = obs + row, *s = syn + row;
    float *a = res + row;
    double *F = scratch + row, *G = F + plane, *QO = G + plane, *QS = QO + plane, *Cc = QS + plane;
    const double dt = (double)dt_f;
    const double w = (double)(weights ? weights[r] * src_weight : 1.0f);

    // ---- 1: the scale, the densities and their CDFs ----
    double m = 0.0;
    for (int i = tid; i < nt; i += kTile) m = fmax(m, (double)fabsf(o[i]));
    const double A = block_all<true>(m, lds);
    if (!(A > 0.0)) {  // a dead trace (the whole block takes the branch)
        for (int i = tid; i < nt; i += kTile) a[i] = 0.0f;
        if (tid == 0) wsum[r] = 0.0;
        return;
    }
    double carry[2] = {0.0, 0.0};
    for (int base = 1; base < nt; base += kTile) {
        const int i = base + tid;
        double v[2] = {0.0, 0.0}, tot[2];
        if (i < nt) {
            QS[i] = v[0] = softplus(beta * (double)s[i] / A);
            QO[i] = v[1] = softplus(beta * (double)o[i] / A);
        }
        block_scan(v, tot, lds);
        if (i < nt) {
            F[i] = carry[0] + v[0];
            G[i] = carry[1] + v[1];
        }
        carry[0] += tot[0];
        carry[1] += tot[1];
    }
    const double Ss = carry[0], So = carry[1];  // the bits of F[nt - 1] and G[nt - 1]: a tile's total is its last thread's prefix
    for (int i = 1 + tid; i < nt; i += kTile) {
        F[i] = F[i] / Ss;
        G[i] = G[i] / So;
    }
    if (tid == 0) G[0] = 0.0;
    __syncthreads();

    // ---- 2: the transport map ----
    double part = 0.0;
    for (int i = 1 + tid; i < nt; i += kTile) {
        const double Fi = F[i];
        int lo = 1, hi = nt - 1;  // the first j in [1, nt - 1] with G[j] >= Fi; G[nt - 1] = 1 >= Fi, and hi is the clamp
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (G[mid] >= Fi)
                hi = mid;
            else
                lo = mid + 1;
        }
        const int j = lo;
        const double gj = QO[j] / So, fi = QS[i] / Ss, ti = (double)i * dt;
        const double T = (double)(j - 1) * dt + dt * (Fi - G[j - 1]) / gj;
        const double d = (ti - T) * (ti - T);
        part += fi * d;
        Cc[i] = 2.0 * fi * (T - ti) * dt / gj;
        F[i] = d;
    }
    const double W = block_all<false>(part, lds);
    __syncthreads();  // c, and the (t - T)^2 in F, before the reversed walk reads them across threads

    // ---- 3: psi = (t - T)^2 + the suffix sums of c, and its mean under f ----
    double tail = 0.0;
    part = 0.0;
    for (int top = nt - 1; top >= 1; top -= kTile) {
        const int i = top - tid;
        double v[1] = {i >= 1 ? Cc[i] : 0.0}, tot[1];
        block_scan(v, tot, lds);
        if (i >= 1) {
            const double psi = F[i] + (tail + v[0]);
            F[i] = psi;
            part += QS[i] / Ss * psi;
        }
        tail += tot[0];
    }
    const double P = block_all<false>(part, lds);

    // ---- 4: the adjoint source, rounded once (the reversed walk again: every thread reads the psi it wrote) ----
    for (int top = nt - 1; top >= 1; top -= kTile) {
        const int i = top - tid;
        if (i < 1) continue;
        const double dWds = sigmoid(beta * (double)s[i] / A) * (beta / A) * ((F[i] - P) / Ss);
        a[i] = (float)(-0.5 * w * dWds);
    }
    if (tid == 0) {
        a[0] = 0.0f;
        wsum[r] = w * W;
    }
}

}  // namespace

void launch_w2_trace(hipStream_t st, int nt, int nrec, const float *obs, const float *syn, float *res, const float *weights, float src_weight,
                     float dt, double beta, double *scratch, size_t plane, double *wsum) {
    hipLaunchKernelGGL(k_w2_trace, dim3(nrec), dim3(kTile), 0, st, nt, obs, syn, res, weights, src_weight, dt, beta, scratch, plane, wsum);
}

}  // namespace sepfwi
