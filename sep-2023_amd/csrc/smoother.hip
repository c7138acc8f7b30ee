// smoother.hip -- the model-space smoothing operator S and its exact transpose (smoother.hpp; the operator is written out in
// include/sepfwi.h, sepfwi_smooth_plan / sepfwi_smooth_apply).
//
// Every kernel is a gather: a thread owns one cell (i, j) of one field and walks the up to 2 r + 1 taps of its row (x pass) or of its
// column (z pass) with shifted global loads.  Along either axis the 64 lanes of a wave read 64 consecutive floats per tap, and the
// rows a block's four waves walk overlap, so the taps are vector-L1 hits; the time goes into the tap weight (one division and one
// exponential per tap), not into the loads, so no LDS halo is staged.  No atomics, no scatter: the same input gives the same bits.
// Tiling of regularizer.hip: 64 lanes along x, 4 rows; blockIdx.z is the field (the axis in the normaliser).
// float32 with one fixed operation list (the build has -ffp-contract=off), sig the axis' width array and r its radius, m = j + t the
// tap's cell along the axis, the taps taken in ascending t from max(-r, -j) to min(r, n - 1 - j):
//     qj = sig(j) sig(j),  qm = sig(m) sig(m),  d = qj + qm                  the same sum from both ends: K is symmetric bit for bit
//     w  = 1 for t = 0,  else  d > 0 ? expf(-((float)(t t) / d)) : 0         (t t <= 4096 is exact; a NaN width gives weight 0)
//     v  = in(m)  (forward)   or   in(m) inv(m)  (transpose);  v = 1 in the normaliser
//     a  = 0, c = 0;  over the taps:  y = w v - c,  s = a + y,  c = (s - a) - y,  a = s         a compensated (Kahan) sum
//     inv(j) = 1 / a  (the normaliser: a = N)        out(j) = a inv(j)  (forward)   or   a  (transpose)
// The compensation keeps the error of a sum of up to 129 terms at one rounding, whatever the radius; and since w 1 = w exactly, the
// gather of a constant field repeats the normaliser's sum bit for bit, which is what holds S 1 within a few roundings of 1.
// An axis without a width array or with radius 0 is the identity and runs no pass.
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>

#include "hip_check.hpp"
#include "model_call.hpp"
#include "smoother.hpp"

namespace sepfwi {

namespace {

struct SmoothArgs {  // by value into the pass kernels
    int nz, nx, r;
    const float *sig, *inv;  // of the pass' axis; both NULL with r = 0: a plain copy
    int pre;                 // 1: scale by inv before the gather (transpose); 0: after it (forward)
    const float *in[3];
    float *out[3];
};

__device__ __forceinline__ float smooth_weight(float qj, float qm, int t) {
    const float d = qj + qm;
    return d > 0.0f ? expf(-((float)(t * t) / d)) : 0.0f;
}

// a += x, compensated: c carries what the additions so far rounded away
__device__ __forceinline__ void smooth_add(float &a, float &c, float x) {
    const float y = x - c, s = a + y;
    c = (s - a) - y;
    a = s;
}

// the cell, its place along the axis and the range of taps that stay inside the grid
struct Walk {
    size_t o;
    long long stride;
    int lo, hi;
};
template <int AXIS>
__device__ __forceinline__ Walk smooth_walk(int nz, int nx, int r, int i, int j) {
    const int pos = AXIS ? i : j, len = AXIS ? nz : nx;
    Walk w;
    w.o = (size_t)i * nx + j;
    w.stride = AXIS ? nx : 1;
    w.lo = -min(r, pos);
    w.hi = min(r, len - 1 - pos);
    return w;
}

template <int AXIS>
__device__ __forceinline__ void smooth_pass(const SmoothArgs &A) {
    const int f = blockIdx.z;
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (!A.in[f] || i >= A.nz || j >= A.nx) return;
    const Walk k = smooth_walk<AXIS>(A.nz, A.nx, A.r, i, j);
    const float *in = A.in[f];  // may be out[f] when r = 0
    float qj = 0.0f;
    if (A.sig) {
        const float s = A.sig[k.o];
        qj = s * s;
    }
    float a = 0.0f, c = 0.0f;
    for (int t = k.lo; t <= k.hi; t++) {
        const size_t m = (size_t)((long long)k.o + t * k.stride);
        float w = 1.0f;
        if (t != 0) {
            const float s = A.sig[m];
            w = smooth_weight(qj, s * s, t);
        }
        float v = in[m];
        if (A.pre) v = v * A.inv[m];
        smooth_add(a, c, w * v);
    }
    if (!A.pre && A.inv) a = a * A.inv[k.o];
    A.out[f][k.o] = a;
}

}  // namespace

// grid (ceil(nx / 64), ceil(nz / 4), 3), block (64, 4): a wave is one row segment; a NULL field's blocks return at once
__global__ void k_smooth_x(SmoothArgs A) { smooth_pass<0>(A); }
__global__ void k_smooth_z(SmoothArgs A) { smooth_pass<1>(A); }

// the same tiles, blockIdx.z the axis (0: x, 1: z): inv = 1 / (the sum of the axis' tap weights); an axis without widths is skipped
__global__ void k_smooth_norm(int nz, int nx, int rx, int rz, const float *__restrict__ sigx, const float *__restrict__ sigz,
                              float *__restrict__ inv_nx, float *__restrict__ inv_nz) {
    const int axis = blockIdx.z;
    const float *__restrict__ sig = axis ? sigz : sigx;
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (!sig || i >= nz || j >= nx) return;
    const Walk k = axis ? smooth_walk<1>(nz, nx, rz, i, j) : smooth_walk<0>(nz, nx, rx, i, j);
    const float s0 = sig[k.o], qj = s0 * s0;
    float n = 0.0f, c = 0.0f;
    for (int t = k.lo; t <= k.hi; t++) {
        float w = 1.0f;
        if (t != 0) {
            const float s = sig[(size_t)((long long)k.o + t * k.stride)];
            w = smooth_weight(qj, s * s, t);
        }
        smooth_add(n, c, w);
    }
    (axis ? inv_nz : inv_nx)[k.o] = 1.0f / n;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
namespace {

void bad(const std::string &what) { throw std::invalid_argument("smoother: " + what); }

void validate(const SmoothGeom &g, const float *inv_nx, const float *inv_nz) {
    if (g.nz < 1 || g.nx < 1) bad("nz and nx must be at least 1");
    if (g.rx < 0 || g.rx > kSmoothMaxRadius || g.rz < 0 || g.rz > kSmoothMaxRadius)
        bad("the radii must lie between 0 and " + std::to_string(kSmoothMaxRadius));
    if (g.sigx && !inv_nx) bad("sigx is given without inv_nx");
    if (g.sigz && !inv_nz) bad("sigz is given without inv_nz");
}

}  // namespace

void run_smooth_plan(const SmoothGeom &g, float *inv_nx, float *inv_nz, hipStream_t st) {
    validate(g, inv_nx, inv_nz);
    if (!g.sigx && !g.sigz) return;
    const size_t n = (size_t)g.nz * (size_t)g.nx;
    ModelCall call("smoother", n, st);
    call.see(g.sigx), call.see(g.sigz), call.see(inv_nx), call.see(inv_nz);
    call.enter();
    const float *sx = call.in(g.sigx), *sz = call.in(g.sigz);
    float *ix = g.sigx ? call.out(inv_nx) : nullptr, *iz = g.sigz ? call.out(inv_nz) : nullptr;
    const dim3 grid((g.nx + 63) / 64, (g.nz + 3) / 4, 2), block(64, 4);
    hipLaunchKernelGGL(k_smooth_norm, grid, block, 0, st, g.nz, g.nx, g.rx, g.rz, sx, sz, ix, iz);
    HIP_OK(hipGetLastError());
    call.finish();
}

void run_smooth_apply(const SmoothGeom &g, const float *inv_nx, const float *inv_nz, bool transpose, const float *const *in,
                      float *const *out, hipStream_t st) {
    validate(g, inv_nx, inv_nz);
    if (!in || !out) bad("the field triples must not be NULL");
    bool any = false;
    for (int k = 0; k < 3; k++) {
        if (in[k] && !out[k]) bad("in[" + std::to_string(k) + "] is given without out[" + std::to_string(k) + "]");
        if (!in[k] && out[k]) bad("out[" + std::to_string(k) + "] is given without in[" + std::to_string(k) + "]");
        any = any || in[k];
    }
    if (!any) bad("all three fields are NULL");
    const size_t n = (size_t)g.nz * (size_t)g.nx;

    ModelCall call("smoother", n, st);
    call.see(g.sigx), call.see(g.sigz), call.see(inv_nx), call.see(inv_nz);
    for (int k = 0; k < 3; k++) call.see(in[k]), call.see(out[k]);
    const int dev = call.enter();

    const bool on_x = g.sigx && g.rx > 0, on_z = g.sigz && g.rz > 0;
    const float *sig[2] = {on_x ? call.in(g.sigx) : nullptr, on_z ? call.in(g.sigz) : nullptr};
    const float *inv[2] = {on_x ? call.in(inv_nx) : nullptr, on_z ? call.in(inv_nz) : nullptr};
    const int radius[2] = {g.rx, g.rz};

    const float *src[3];  // (a host array given as input and output is staged twice: the passes then run out of place)
    float *dst[3];
    for (int k = 0; k < 3; k++) src[k] = call.in(in[k]), dst[k] = call.out(out[k]);

    // S = Sx Sz runs the z pass first, S^T = Sz^T Sx^T the x pass; an identity axis runs none
    int axes[2], passes = 0;
    for (int a : {transpose ? 0 : 1, transpose ? 1 : 0})
        if (a == 0 ? on_x : on_z) axes[passes++] = a;
    bool aliased = false, same = true;  // an output that is some input; every output its own input
    for (int k = 0; k < 3; k++) {
        if (!src[k]) continue;
        same = same && src[k] == dst[k];
        for (int l = 0; l < 3; l++) aliased = aliased || (src[l] && src[l] == dst[k]);
    }

    const dim3 grid((g.nx + 63) / 64, (g.nz + 3) / 4, 3), block(64, 4);
    auto launch = [&](int axis, int r, const float *const *from, float *const *to) {  // r = 0: a copy, cell by cell
        SmoothArgs A{};
        A.nz = g.nz, A.nx = g.nx, A.r = r;
        A.sig = r > 0 ? sig[axis] : nullptr, A.inv = r > 0 ? inv[axis] : nullptr;
        A.pre = (transpose && r > 0) ? 1 : 0;
        for (int k = 0; k < 3; k++) A.in[k] = src[k] ? from[k] : nullptr, A.out[k] = src[k] ? to[k] : nullptr;
        if (axis == 0)
            hipLaunchKernelGGL(k_smooth_x, grid, block, 0, st, A);
        else
            hipLaunchKernelGGL(k_smooth_z, grid, block, 0, st, A);
    };
    // no pass: a copy, cell by cell (radius 0).  A gather must not read what its own launch writes, so a call whose outputs are
    // inputs goes through the intermediate, with a copy behind a single pass.
    const int first = passes ? axes[0] : 0, r_first = passes ? radius[first] : 0;
    if (passes == 0 && same) {
        // S = I in place: nothing to do
    } else if (passes <= 1 && !aliased) {
        launch(first, r_first, src, dst);
    } else {
        float *mid[3];  // three fields: what the first pass hands to the second
        mid[0] = model_workspace<float>(ModelOp::Smoother, dev, st, 3 * n);
        mid[1] = mid[0] + n, mid[2] = mid[1] + n;
        launch(first, r_first, src, mid);
        if (passes == 2)
            launch(axes[1], radius[axes[1]], mid, dst);
        else
            launch(0, 0, mid, dst);
    }
    HIP_OK(hipGetLastError());
    call.finish();
}

}  // namespace sepfwi
