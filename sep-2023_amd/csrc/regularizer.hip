// regularizer.hip -- model-space regularisation (regularizer.hpp; the functional is written out in include/sepfwi.h).
//
// Both kernels are gathers: a thread owns one cell (i, j) of one field and needs the flux of its own cell and of its two
// predecessors (i, j-1) and (i-1, j), each formed from shifted global loads that hit the vector L1 -- no LDS halo (README: staging
// halos measured slower than shifted loads here), no atomics, no scatter.  Tiling of param_maps.hip: 64 lanes along x, 4 rows;
// blockIdx.z is the field.  float32 with one fixed operation list (the build has -ffp-contract=off):
//     rx = 1 / (s dx), rz = 1 / (s dz), a2 = alpha / s^2, e2 = eps^2         formed in double on the host, rounded once
//     gx = (p(i,j+1) - p(i,j)) rx,  gz = (p(i+1,j) - p(i,j)) rz              0 in the last column / row
//     n2 = gx gx + gz gz,  phi = sqrt(n2 + e2)                               only when gamma > 0 (or for the energy)
//     c  = W (beta + gamma / phi),  fx = c gx,  fz = c gz                    W of the cell that OWNS the flux
//     g  = ((((W a2) (p - p0) - fx rx) - fz rz) + fx(i,j-1) rx) + fz(i-1,j) rz
//     energy = W ((a2/2) (p - p0)^2 + ((beta/2) n2 + gamma (n2 / (phi + eps))))
// phi - eps is evaluated as n2 / (phi + eps): the same number without the cancellation, so every term of the energy is a
// non-negative float32 with a relative error of a few roundings, exactly 0 for a constant field.
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

#include "hip_check.hpp"
#include "model_call.hpp"
#include "regularizer.hpp"

namespace sepfwi {

namespace {

struct RegArgs {  // by value into the kernels
    int nz, nx;
    const float *p[3], *p0[3], *v[3], *W;
    float *out[3];
    float a2[3], beta[3], gamma[3], rx[3], rz[3];
    float eps, e2;
};

struct Pair {
    float x, z;
};

// forward differences of `a` at the existing cell (i, j), scaled
__device__ __forceinline__ Pair reg_diff(const float *__restrict__ a, int nz, int nx, int i, int j, float rx, float rz) {
    const size_t o = (size_t)i * nx + j;
    const float c = a[o];
    Pair d;
    d.x = j + 1 < nx ? (a[o + 1] - c) * rx : 0.0f;
    d.z = i + 1 < nz ? (a[o + nx] - c) * rz : 0.0f;
    return d;
}

// the flux (fx, fz) = W (beta + gamma / phi) (gx, gz) of the existing cell (i, j)
__device__ __forceinline__ Pair reg_flux(const RegArgs &A, int f, int i, int j) {
    const Pair g = reg_diff(A.p[f], A.nz, A.nx, i, j, A.rx[f], A.rz[f]);
    float c = A.beta[f];
    if (A.gamma[f] > 0.0f) c = c + A.gamma[f] / sqrtf((g.x * g.x + g.z * g.z) + A.e2);
    c = (A.W ? A.W[(size_t)i * A.nx + j] : 1.0f) * c;
    Pair o;
    o.x = c * g.x;
    o.z = c * g.z;
    return o;
}

// its directional derivative along v, q the differences of v: t = W (beta q + gamma (q / phi - g (g.q) / phi^3)), with the bracket
// written as (eps^2 q + (-gz, gx) c) / phi^3, c = gx qz - gz qx -- the same number, since phi^2 q - g (g.q) = eps^2 q + |g|^2 q - g (g.q),
// without the cancellation of q against its own projection where eps is small against |g| (on a single row or column c is exactly 0),
// and v^T H v = sum W (beta |q|^2 + gamma (eps^2 |q|^2 + c^2) / phi^3) is visibly non-negative
__device__ __forceinline__ Pair reg_dflux(const RegArgs &A, int f, int i, int j) {
    const Pair q = reg_diff(A.v[f], A.nz, A.nx, i, j, A.rx[f], A.rz[f]);
    Pair t;
    t.x = A.beta[f] * q.x;
    t.z = A.beta[f] * q.z;
    if (A.gamma[f] > 0.0f) {
        const Pair g = reg_diff(A.p[f], A.nz, A.nx, i, j, A.rx[f], A.rz[f]);
        const float iphi = 1.0f / sqrtf((g.x * g.x + g.z * g.z) + A.e2);
        const float iphi3 = (iphi * iphi) * iphi, c = g.x * q.z - g.z * q.x;
        t.x = t.x + A.gamma[f] * ((A.e2 * q.x - g.z * c) * iphi3);
        t.z = t.z + A.gamma[f] * ((A.e2 * q.z + g.x * c) * iphi3);
    }
    const float w = A.W ? A.W[(size_t)i * A.nx + j] : 1.0f;
    t.x = w * t.x;
    t.z = w * t.z;
    return t;
}

}  // namespace

// grid (ceil(nx / 64), ceil(nz / 4), 3), block (64, 4): a wave is one row segment.  partial (may be NULL): one double per block,
// [field][block row][block column]; a skipped field's blocks write 0.
__global__ void k_reg_value_grad(RegArgs A, double *__restrict__ partial) {
    const int f = blockIdx.z;
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    float e = 0.0f;
    if (A.p[f] && i < A.nz && j < A.nx) {
        const float *__restrict__ p = A.p[f];
        const size_t o = (size_t)i * A.nx + j;
        const float w = A.W ? A.W[o] : 1.0f;
        const float rx = A.rx[f], rz = A.rz[f];
        float t0 = 0.0f;
        if (A.a2[f] > 0.0f) {
            const float d = p[o] - A.p0[f][o];
            t0 = (w * A.a2[f]) * d;
            e = (0.5f * A.a2[f]) * (d * d);
        }
        if (partial && (A.beta[f] > 0.0f || A.gamma[f] > 0.0f)) {
            const Pair g = reg_diff(p, A.nz, A.nx, i, j, rx, rz);
            const float n2 = g.x * g.x + g.z * g.z;
            float et = (0.5f * A.beta[f]) * n2;
            if (A.gamma[f] > 0.0f) et = et + A.gamma[f] * (n2 / (sqrtf(n2 + A.e2) + A.eps));
            e = e + et;
        }
        e = w * e;
        if (A.out[f]) {
            const Pair own = reg_flux(A, f, i, j);
            float g = (t0 - own.x * rx) - own.z * rz;
            g = g + (j > 0 ? reg_flux(A, f, i, j - 1).x * rx : 0.0f);
            g = g + (i > 0 ? reg_flux(A, f, i - 1, j).z * rz : 0.0f);
            A.out[f][o] = g;
        }
    }
    if (!partial) return;
    double acc = (double)e;
    // (the tree of dev::wave_sum, written out here and in k_reg_sum: through the helper the compiler orders the same instructions
    // differently, and these kernels' code is held fixed)
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ double part[4];
    if (threadIdx.x == 0) part[threadIdx.y] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partial[((size_t)f * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// *value = sum of the block partials, one block of 1024, a fixed order: the same input gives the same bits.  Four independent
// accumulators per thread keep four loads in flight (one chain of dependent loads took 24 us for the 24 000 partials of three
// 1000 x 2000 fields).
__global__ void k_reg_sum(int n, const double *__restrict__ partial, double *__restrict__ value) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int r = threadIdx.x;
    for (; r + 3 * 1024 < n; r += 4 * 1024) {
        s0 += partial[r];
        s1 += partial[r + 1024];
        s2 += partial[r + 2 * 1024];
        s3 += partial[r + 3 * 1024];
    }
    for (; r < n; r += 1024) s0 += partial[r];
    double s = (s0 + s1) + (s2 + s3);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    __shared__ double part[16];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < 16; k++) t += part[k];
        *value = t;
    }
}

// the same grid; a field without p or without v is skipped (its hv is zero-filled by the host)
__global__ void k_reg_hvp(RegArgs A) {
    const int f = blockIdx.z;
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (!A.p[f] || !A.v[f] || !A.out[f] || i >= A.nz || j >= A.nx) return;
    const size_t o = (size_t)i * A.nx + j;
    const float w = A.W ? A.W[o] : 1.0f;
    const float rx = A.rx[f], rz = A.rz[f];
    const float t0 = A.a2[f] > 0.0f ? (w * A.a2[f]) * A.v[f][o] : 0.0f;
    const Pair own = reg_dflux(A, f, i, j);
    float h = (t0 - own.x * rx) - own.z * rz;
    h = h + (j > 0 ? reg_dflux(A, f, i, j - 1).x * rx : 0.0f);
    h = h + (i > 0 ? reg_dflux(A, f, i - 1, j).z * rz : 0.0f);
    A.out[f][o] = h;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
namespace {

void validate(const RegModel &m, const float *const *v, double *value, float *const *out) {
    auto bad = [](const std::string &what) { throw std::invalid_argument("regularizer: " + what); };
    if (m.nz < 1 || m.nx < 1) bad("nz and nx must be at least 1");
    if (!m.p || !m.p0 || !m.alpha || !m.beta || !m.gamma || !m.scale) bad("the argument triples must not be NULL");
    if (!(m.dx > 0.0f) || !(m.dz > 0.0f) || !std::isfinite(m.dx) || !std::isfinite(m.dz)) bad("dx and dz must be positive");
    bool any = false, tv = false;
    for (int k = 0; k < 3; k++) {
        if (v && v[k] && !m.p[k]) bad("v[" + std::to_string(k) + "] is given for a field without p");
        if (!m.p[k]) continue;
        any = true;
        for (float wgt : {m.alpha[k], m.beta[k], m.gamma[k]})
            if (!std::isfinite(wgt) || wgt < 0.0f) bad("alpha, beta and gamma must be finite and non-negative");
        if (!(m.scale[k] > 0.0f) || !std::isfinite(m.scale[k])) bad("scale must be positive");
        if (m.alpha[k] > 0.0f && !m.p0[k]) bad("a field with alpha > 0 needs its prior p0");
        tv = tv || m.gamma[k] > 0.0f;
    }
    if (!any) bad("all three fields are NULL");
    if (tv && (!(m.eps > 0.0f) || !std::isfinite(m.eps))) bad("eps must be positive when a gamma is");
    if (v && (!out || value)) bad("the product needs hv and computes no value");
}

}  // namespace

void run_regularizer(const RegModel &m, const float *const *v, double *value, float *const *out, hipStream_t st) {
    validate(m, v, value, out);
    const bool product = v != nullptr;
    const size_t n = (size_t)m.nz * (size_t)m.nx;

    ModelCall call("regularizer", n, st);
    call.see(m.W), call.see(value);
    for (int k = 0; k < 3; k++) {
        call.see(m.p[k]), call.see(m.p0[k]);
        if (v) call.see(v[k]);
        if (out) call.see(out[k]);
    }
    const int dev = call.enter();

    RegArgs A{};
    A.nz = m.nz, A.nx = m.nx;
    A.W = call.in(m.W);
    A.eps = m.eps;
    A.e2 = (float)((double)m.eps * (double)m.eps);
    for (int k = 0; k < 3; k++) {
        const bool on = m.p[k] && (!product || v[k]);
        if (out && out[k] && !on) {  // a field that is skipped: zeros
            if (call.on_device(out[k]))
                HIP_OK(hipMemsetAsync(out[k], 0, n * sizeof(float), st));
            else
                std::fill(out[k], out[k] + n, 0.0f);
        }
        if (!on) continue;
        const double s = (double)m.scale[k];
        A.p[k] = call.in(m.p[k]);
        A.p0[k] = m.alpha[k] > 0.0f ? call.in(m.p0[k]) : nullptr;
        A.v[k] = product ? call.in(v[k]) : nullptr;
        A.a2[k] = (float)((double)m.alpha[k] / (s * s));
        A.beta[k] = m.beta[k], A.gamma[k] = m.gamma[k];
        A.rx[k] = (float)(1.0 / (s * (double)m.dx));
        A.rz[k] = (float)(1.0 / (s * (double)m.dz));
        if (out) A.out[k] = call.out(out[k]);
    }

    const dim3 grid((m.nx + 63) / 64, (m.nz + 3) / 4, 3), block(64, 4);
    if (product) {
        hipLaunchKernelGGL(k_reg_hvp, grid, block, 0, st, A);
    } else {
        double *partial = nullptr;
        const size_t blocks = (size_t)grid.x * grid.y * grid.z;
        if (value) partial = model_workspace<double>(ModelOp::Regularizer, dev, st, blocks + 1);  // the block partials, then the value
        hipLaunchKernelGGL(k_reg_value_grad, grid, block, 0, st, A, partial);
        if (value) {
            double *dvalue = call.on_device(value) ? value : partial + blocks;
            hipLaunchKernelGGL(k_reg_sum, dim3(1), dim3(1024), 0, st, (int)blocks, (const double *)partial, dvalue);
            if (dvalue != value) call.host_result(value, dvalue, sizeof(double));
        }
    }
    HIP_OK(hipGetLastError());
    call.finish();
}

}  // namespace sepfwi
