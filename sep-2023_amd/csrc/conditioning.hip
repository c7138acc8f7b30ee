// conditioning.hip -- the data-conditioning chain of the misfit: time windows with trace weights, zero-phase band-pass
// (hipFFT), apparent-slowness (f-k) fan filter across the channels, normalised zero-lag cross-correlation misfit and its adjoint source.
//
// In the reference these are utilities.cu:733-1111 (kernels) and :1115-1166 (bp_filter1d, cuFFT); every call site in the
// driver is commented out (libCUFD.cu:353-457), so the chain is DORMANT there: the parameter keys are parsed and nothing
// happens.  Here a key that is set switches its stage on, composed in the order of those commented lines:
//     window(obs), window(syn)  ->  band-pass(obs), band-pass(syn)  ->  [source-signature update of syn]  ->  misfit / residual
//     ->  [its transpose on res]  ->  band-pass(res)  ->  window(res)
// applied to the axial-strain gathers (the component that enters misfit and adjoint source, libCUFD.cu:427,607).  Traces
// are processed in the files' [rec][it] layout.  Parity for this extension is against the numpy restatement in
// oracle/oracle.py (cond_window, cond_bandpass, conditioned_residual); the reference offers no run of it to pin on.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>  // types and enumerators only: the library itself is opened on first use (FftApi below)

#include <stdexcept>
#include <string>

#include "conditioning.hpp"
#include "device_alloc.hpp"
#include "robust_misfit.hpp"
#include "w2_misfit.hpp"

namespace sepfwi {

namespace {

constexpr double kPi = 3.141592653589793238462643383279502884197169;  // utilities.h:15

// sin / cos ramp of cuda_window (utilities.cu:821-829) and cuda_bp_filter1d (:747-757): float arguments, double sin / cos
__device__ __forceinline__ float ramp(float t, float t0, float t1, float t2, float t3) {
    if (t >= t0 && t < t1) return (float)sin(kPi / 2.0 * (double)(t - t0) / (double)(t1 - t0));
    if (t >= t1 && t < t2) return 1.0f;
    if (t >= t2 && t < t3) return (float)cos(kPi / 2.0 * (double)(t - t2) / (double)(t3 - t2));
    return 0.0f;
}

// The block reduction of every sum below: v[n] summed over a block of 256 threads (four waves), N sums side by side.  Per sum the 64-lane
// shuffle tree, one partial per wave in LDS, then part[0] + part[1] + part[2] + part[3] -- in THAT order, which is what keeps the misfits
// and norms the same bits from one build to the next.  The result is meant for thread 0; one use per kernel (nothing guards `part` against a
// second round).
template <int N> __device__ __forceinline__ void block_sum(double (&v)[N]) {
    __shared__ double part[N][4];
    for (int n = 0; n < N; n++) {
        for (int off = 32; off > 0; off >>= 1) v[n] += __shfl_down(v[n], off, 64);
        if ((threadIdx.x & 63) == 0) part[n][threadIdx.x >> 6] = v[n];
    }
    __syncthreads();
    for (int n = 0; n < N; n++) v[n] = part[n][0] + part[n][1] + part[n][2] + part[n][3];
}
__device__ __forceinline__ double block_sum(double v) {
    double one[1] = {v};
    block_sum(one);
    return one[0];
}

// cuda_window, both overloads (utilities.cu:787-884).  win_start == nullptr: one taper of `ratio` of the trace length at
// both ends; else per-trace window [win_start, win_end] seconds, amplitude times weights[r] * src_weight.
__global__ void k_window(int nt, int nrec, float dt, const float *__restrict__ win_start, const float *__restrict__ win_end,
                         const float *__restrict__ weights, float src_weight, float ratio, float *__restrict__ data) {
    const int it = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (it >= nt || r >= nrec) return;
    const float t = (float)it * dt;
    float t0 = 0.0f, t3 = (float)nt * dt, offset;
    if (win_start) {
        const float t_max = (float)nt * dt;
        t0 = fminf(fmaxf(win_start[r], 0.0f), t_max);
        t3 = fminf(fmaxf(win_end[r], 0.0f), t_max);
        offset = (t3 - t0) * ratio;
        if (offset <= 0.0f) return;  // "Window error 1": trace untouched
    } else {
        offset = (float)nt * dt * ratio;
        if (2.0 * (double)offset >= (double)(t3 - t0)) return;  // "Window error 2"
    }
    const float a = ramp(t, t0, t0 + offset, t3 - offset, t3);
    const size_t i = (size_t)r * nt + it;
    data[i] = win_start ? data[i] * (a * a) * weights[r] * src_weight : data[i] * (a * a);
}

// embed [rec][nt] into zeroed [rec][2 nt] / crop back with the 1 / (2 nt) scale of the unnormalised inverse transform
__global__ void k_embed(int nt, int nrec, const float *__restrict__ data, float *__restrict__ pad) {
    const int it = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (it >= 2 * nt || r >= nrec) return;
    pad[(size_t)r * 2 * nt + it] = it < nt ? data[(size_t)r * nt + it] : 0.0f;
}
__global__ void k_crop(int nt, int nrec, float *__restrict__ data, const float *__restrict__ pad, float scale) {
    const int it = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (it >= nt || r >= nrec) return;
    data[(size_t)r * nt + it] = pad[(size_t)r * 2 * nt + it] * scale;
}

// cuda_bp_filter1d (utilities.cu:733-760) on nf = nt_pad / 2 + 1 bins per trace
__global__ void k_bp_filter(int nf, int nrec, float df, float f0, float f1, float f2, float f3, hipfftComplex *__restrict__ spec) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (k >= nf || r >= nrec) return;
    const float a = ramp((float)k * df, f0, f1, f2, f3);
    hipfftComplex &c = spec[(size_t)r * nf + k];
    c.x *= a * a;
    c.y *= a * a;
}

// cuda_find_normfact (utilities.cu:1010-1040): out[r] = sum_t a b + DIVCONST; one block per trace, double partial sums, and the norm is
// KEPT in double: k_cross_adjoint subtracts (n_os / n_ss) syn from obs, and where the data nearly fit (obs close to a multiple of syn,
// every late iteration of an inversion) that difference is a cancellation -- a norm rounded to float32 is off by 6e-8 of itself, and
// 6e-8 |obs| is 1e-3 of a residual that is 1e-4 of the data (tests/test_gpu_cross_data.py: nearly fitting data).
__global__ void k_normfact(int nt, const float *__restrict__ a, const float *__restrict__ b, double *__restrict__ out) {
    const int r = blockIdx.x;
    double s = 0.0;
    for (int it = threadIdx.x; it < nt; it += blockDim.x) s += (double)a[(size_t)r * nt + it] * (double)b[(size_t)r * nt + it];
    s = block_sum(s);
    if (threadIdx.x == 0) out[r] = s + (double)1e-9f;  // DIVCONST, utilities.h:24
}

// cuda_normal_misfit (utilities.cu:1056-1083): *acc += -2 sum_r cross / (sqrt(obs) sqrt(cal)) w_r  (the driver halves the total)
__global__ void k_cross_misfit(int nrec, const double *__restrict__ n_os, const double *__restrict__ n_oo, const double *__restrict__ n_ss,
                               const float *__restrict__ weights, float src_weight, double *__restrict__ acc) {
    double s = 0.0;
    for (int r = threadIdx.x; r < nrec; r += blockDim.x)
        s += n_os[r] / (sqrt(n_oo[r]) * sqrt(n_ss[r])) * (double)(weights ? weights[r] * src_weight : 1.0f);
    s = block_sum(s);
    if (threadIdx.x == 0) atomicAdd(acc, -2.0 * s);
}

// cuda_normal_adjoint_source (utilities.cu:1086-1111).  obs - (n_os / n_ss) syn is formed per element in double, from the double
// norms, and rounded once: its error is then half a unit of the residual's last place, however nearly the data fit.
__global__ void k_cross_adjoint(int nt, int nrec, const double *__restrict__ n_oo, const double *__restrict__ n_ss,
                                const double *__restrict__ n_os, const float *__restrict__ obs, const float *__restrict__ syn,
                                float *__restrict__ res, const float *__restrict__ weights, float src_weight) {
    const int it = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (it >= nt || r >= nrec) return;
    const size_t i = (size_t)r * nt + it;
    const double w = (double)(weights ? weights[r] * src_weight : 1.0f);
    const double ratio = n_os[r] / n_ss[r], scale = w / (sqrt(n_oo[r]) * sqrt(n_ss[r]));
    res[i] = (float)(((double)obs[i] - ratio * (double)syn[i]) * scale);
}

// gpuMinus + cuda_cal_objective on [rec][it] (utilities.cu:154-205): r = obs - syn, first sample zeroed, *acc += sum r^2
__global__ void k_l2_residual(int nt, int nrec, const float *__restrict__ obs, const float *__restrict__ syn, float *__restrict__ res,
                              double *__restrict__ acc) {
    const int r = blockIdx.x;
    double s = 0.0;
    for (int it = threadIdx.x; it < nt; it += blockDim.x) {
        const size_t i = (size_t)r * nt + it;
        const float v = it == 0 ? 0.0f : obs[i] - syn[i];
        res[i] = v;
        s += (double)v * (double)v;
    }
    s = block_sum(s);
    if (threadIdx.x == 0) atomicAdd(acc, s);
}

// the same residual for observed data syn - d (the Gauss-Newton product, d = C J v): r = -d, first sample zeroed.  No misfit.
// (sign = -1; sepfwi_data_gn hands out +Z d: sign = 1.  A product with -1 is the negation, bit for bit.)
__global__ void k_scattered_residual(int nt, int nrec, const float *__restrict__ d, float *__restrict__ res, float sign) {
    const int it = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (it >= nt || r >= nrec) return;
    const size_t i = (size_t)r * nt + it;
    res[i] = it == 0 ? 0.0f : sign * d[i];
}

// cuda_spectrum_update (utilities.cu:905-977), first half: one block per frequency bin sums conj(C_r) O_r and |C_r|^2 over the
// channels (double partial sums; the reference: 512 strided float partials and a tree) and divides:
// coef = num / (den + lambda), lambda = 1e-6 added to the real denominator.
__global__ void k_matching_coef(int nf, int nrec, const hipfftComplex *__restrict__ O, const hipfftComplex *__restrict__ Cs,
                                hipfftComplex *__restrict__ coef) {
    const int k = blockIdx.x;
    double s[3] = {0.0, 0.0, 0.0};  // Re and Im of the numerator, the denominator
    for (int r = threadIdx.x; r < nrec; r += blockDim.x) {
        const hipfftComplex o = O[(size_t)r * nf + k], c = Cs[(size_t)r * nf + k];
        s[0] += (double)c.x * o.x + (double)c.y * o.y;   // conj(c) * o
        s[1] += (double)c.x * o.y - (double)c.y * o.x;
        s[2] += (double)c.x * c.x + (double)c.y * c.y;
    }
    block_sum(s);
    if (threadIdx.x == 0) {
        const double d = s[2] + 1e-6;
        coef[k].x = (float)(s[0] / d);
        coef[k].y = (float)(s[1] / d);
    }
}

// spectra times the per-frequency coefficient (second half of cuda_spectrum_update; cuda_filter1d, utilities.cu:765-773), or times
// its conjugate (the transpose)
__global__ void k_apply_coef(int nf, int nrec, hipfftComplex *__restrict__ spec, const hipfftComplex *__restrict__ coef, int conj) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (k >= nf || r >= nrec) return;
    const float cr = coef[k].x, ci = conj ? -coef[k].y : coef[k].y;
    hipfftComplex &v = spec[(size_t)r * nf + k];
    const float x = v.x * cr - v.y * ci, y = v.x * ci + v.y * cr;
    v.x = x;
    v.y = y;
}

// ---- envelope misfit (parameter key if_envelope_misfit; no counterpart in the reference) ------------------------------------------
// Spectrum multiplier of the discrete Hilbert transform on the nf = nt + 1 bins of a trace zero-padded to 2 nt: bin k times -i for
// 0 < k < nt, times 0 for k = 0 and the Nyquist bin k = nt.  With pad and crop around it the transform is exactly antisymmetric.
__global__ void k_hilbert_mult(int nf, int nrec, hipfftComplex *__restrict__ spec) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (k >= nf || r >= nrec) return;
    hipfftComplex &c = spec[(size_t)r * nf + k];
    const bool keep = k > 0 && k < nf - 1;
    const float x = c.x, y = c.y;
    c.x = keep ? y : 0.0f;  // (x + i y) (-i) = y - i x
    c.y = keep ? -x : 0.0f;
}

// d = o - s: the data residual whose Hilbert transform k_env_residual needs
__global__ void k_env_diff(int nt, int nrec, const float *__restrict__ o, const float *__restrict__ s, float *__restrict__ d) {
    const int it = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (it >= nt || r >= nrec) return;
    const size_t i = (size_t)r * nt + it;
    d[i] = o[i] - s[i];
}

// One block per trace: rho = Z (e(o) - e(s)) with e(x) = x^2 + (H x)^2 and Z the zeroing of sample 0; the trace's sum rho^2 in double
// (the reduction of k_l2_residual) into sum[r] -- no atomics, so that the order of the additions is fixed (k_env_sum adds the traces);
// a = s rho and b = (H s) rho, the two halves of D^T rho = 2 [a - H b].
// rho is formed from the data residual, never as the difference of the two envelopes: with d = o - s and H linear,
//     e(o) - e(s) = d (o + s) + (H d) (H d + 2 H s),
// whose rounding error is a few eps of rho itself.  (e(o) - e(s) taken literally in float32 is off by eps |e(s)|, and where the data
// nearly fit -- |rho| / |e(s)| is 1e-4 on a channel of seed 0 and 1.6e-7 on a shot of seed 10 of tests/test_gpu_envelope_fuzz.py -- that
// was 5e-3 of the adjoint source, and all of it.)  float32 throughout: rho is of the data's second power, a and b of its third, and
// nothing rescales them.
__global__ void k_env_residual(int nt, const float *__restrict__ o, const float *__restrict__ hd, const float *__restrict__ s,
                               const float *__restrict__ hs, float *__restrict__ a, float *__restrict__ b, double *__restrict__ sum) {
    const int r = blockIdx.x;
    double acc = 0.0;
    for (int it = threadIdx.x; it < nt; it += blockDim.x) {
        const size_t i = (size_t)r * nt + it;
        const float ov = o[i], sv = s[i], hv = hs[i], hdv = hd[i];
        const float rho = it == 0 ? 0.0f : (ov - sv) * (ov + sv) + hdv * (hdv + 2.0f * hv);
        a[i] = sv * rho;
        b[i] = hv * rho;
        acc += (double)rho * (double)rho;
    }
    acc = block_sum(acc);
    if (threadIdx.x == 0) sum[r] = acc;
}

// *acc += sum_r sum[r], one block, a fixed order (the call's stream serialises the shots: no atomic is needed)
__global__ void k_env_sum(int nrec, const double *__restrict__ sum, double *__restrict__ acc) {
    double s = 0.0;
    for (int r = threadIdx.x; r < nrec; r += blockDim.x) s += sum[r];
    s = block_sum(s);
    if (threadIdx.x == 0) *acc += s;
}

// The linearised twin at the background s for a data perturbation d: rho' = Z 2 (s d + (H s)(H d)) = Z D d, then a = s rho', b = (H s) rho'
__global__ void k_env_linear(int nt, int nrec, const float *__restrict__ s, const float *__restrict__ hs, const float *__restrict__ d,
                             const float *__restrict__ hd, float *__restrict__ a, float *__restrict__ b) {
    const int it = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (it >= nt || r >= nrec) return;
    const size_t i = (size_t)r * nt + it;
    const float sv = s[i], hv = hs[i];
    const float rho = it == 0 ? 0.0f : 2.0f * (sv * d[i] + hv * hd[i]);
    a[i] = sv * rho;
    b[i] = hv * rho;
}

// a <- sign 2 (a - hb): D^T rho from its two halves (hb = H b), in place
__global__ void k_env_combine(int nt, int nrec, float *__restrict__ a, const float *__restrict__ hb, float sign) {
    const int it = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (it >= nt || r >= nrec) return;
    const size_t i = (size_t)r * nt + it;
    a[i] = sign * (2.0f * (a[i] - hb[i]));
}

// ---- apparent-slowness (f-k) fan filter (parameter keys fk_slowness / fk_mode; no counterpart in the reference) ----------------------------
// The two transpositions between the time-axis and the channel-axis transforms.  Tiles of 32 x 32 float2 in LDS, 256 threads as 32 x 8: the
// global reads and writes both run along the contiguous index of their array (a row of 32 float2 is 256 B), and the tile's pitch of 33
// float2 puts the 32 lanes of a column read (ds_read_b64: banks (a / 4) mod 64 per half wave) on addresses 66 dwords apart, i.e. on 32
// different bank pairs.
//   to channels: spec [nrec][nf] -> specT [nf][P], the rows nrec ... P - 1 of the channel padding written as zeros
//   to traces:   specT [nf][P] -> spec [nrec][nf], the padding rows dropped
constexpr int kFkTile = 32;
__global__ void k_fk_to_channels(int nf, int nrec, int P, const float2 *__restrict__ spec, float2 *__restrict__ specT) {
    __shared__ float2 tile[kFkTile][kFkTile + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int j0 = blockIdx.x * kFkTile, m0 = blockIdx.y * kFkTile;
    for (int i = ty; i < kFkTile; i += 8) {
        const int r = m0 + i, j = j0 + tx;
        tile[i][tx] = (r < nrec && j < nf) ? spec[(size_t)r * nf + j] : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    for (int i = ty; i < kFkTile; i += 8) {
        const int j = j0 + i, m = m0 + tx;
        if (j < nf && m < P) specT[(size_t)j * P + m] = tile[tx][i];
    }
}
__global__ void k_fk_to_traces(int nf, int nrec, int P, const float2 *__restrict__ specT, float2 *__restrict__ spec) {
    __shared__ float2 tile[kFkTile][kFkTile + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int j0 = blockIdx.x * kFkTile, m0 = blockIdx.y * kFkTile;
    for (int i = ty; i < kFkTile; i += 8) {
        const int j = j0 + i, m = m0 + tx;
        tile[i][tx] = (j < nf && m < P) ? specT[(size_t)j * P + m] : make_float2(0.0f, 0.0f);
    }
    __syncthreads();
    for (int i = ty; i < kFkTile; i += 8) {
        const int r = m0 + i, j = j0 + tx;
        if (r < nrec && j < nf) spec[(size_t)r * nf + j] = tile[tx][i];
    }
}

// the trapezoid T(p): 0 outside (p1, p4) (also at p = +-infinity), 1 on [p2, p3], sin^2 / cos^2 ramps between
__device__ __forceinline__ double fk_trapezoid(double p, double p1, double p2, double p3, double p4) {
    if (!(p > p1 && p < p4)) return 0.0;
    if (p < p2) {
        const double s = sin(kPi / 2.0 * (p - p1) / (p2 - p1));
        return s * s;
    }
    if (p <= p3) return 1.0;
    const double c = cos(kPi / 2.0 * (p - p3) / (p4 - p3));
    return c * c;
}

// One thread per bin (j, m) of specT [nt + 1][P]: times the gain of the bin's apparent slowness p = -k_m / f_j = -ms slope / j, ms the signed
// wavenumber index and slope = 2 nt dt / (P delta).  Row j = 0: p = 0 at m = 0, infinite elsewhere.  Time-Nyquist row j = nt and
// wavenumber-Nyquist column m = P / 2: (T(p) + T(-p)) / 2.  Double throughout, the gain rounded once.
__global__ void k_fk_gain(int nt, int P, double slope, double p1, double p2, double p3, double p4, int reject, float2 *__restrict__ specT) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ((size_t)nt + 1) * (size_t)P) return;
    const int j = (int)(i / (size_t)P), m = (int)(i % (size_t)P);
    const int ms = m <= P / 2 ? m : m - P;
    double T;
    if (j == 0) {
        T = ms == 0 ? fk_trapezoid(0.0, p1, p2, p3, p4) : 0.0;
    } else {
        const double p = -(double)ms * slope / (double)j;
        T = fk_trapezoid(p, p1, p2, p3, p4);
        if (j == nt || m == P / 2) T = 0.5 * (T + fk_trapezoid(-p, p1, p2, p3, p4));
    }
    const float g = (float)(reject ? 1.0 - T : T);
    float2 &c = specT[i];
    c.x *= g;
    c.y *= g;
}

// hipFFT is only needed by a parameter file with a band-pass or a source-signature update, so libsepfwi.so does not link it:
// the entry points are resolved with dlopen when the first plan is made, and a ROCm image without hipFFT still loads and
// runs the propagator (a parameter file that asks for a filter then fails with a message that names the library).
struct FftApi {
    hipfftResult (*Plan1d)(hipfftHandle *, int, hipfftType, int);
    hipfftResult (*SetStream)(hipfftHandle, hipStream_t);
    hipfftResult (*ExecR2C)(hipfftHandle, hipfftReal *, hipfftComplex *);
    hipfftResult (*ExecC2R)(hipfftHandle, hipfftComplex *, hipfftReal *);
    hipfftResult (*ExecC2C)(hipfftHandle, hipfftComplex *, hipfftComplex *, int);
    hipfftResult (*Destroy)(hipfftHandle);
};
const FftApi &fft() {
    static const FftApi api = [] {
        void *h = nullptr;
        for (const char *name : {"libhipfft.so.0", "libhipfft.so", "/opt/rocm/lib/libhipfft.so.0"})
            if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) throw std::runtime_error("data conditioning (filter / if_src_update / if_envelope_misfit / fk_slowness) needs hipFFT, and libhipfft.so could not be opened");
        FftApi a{};
        auto sym = [&](const char *n) {
            void *p = dlsym(h, n);
            if (!p) throw std::runtime_error(std::string("libhipfft.so lacks ") + n);
            return p;
        };
        a.Plan1d = (decltype(a.Plan1d))sym("hipfftPlan1d");
        a.SetStream = (decltype(a.SetStream))sym("hipfftSetStream");
        a.ExecR2C = (decltype(a.ExecR2C))sym("hipfftExecR2C");
        a.ExecC2R = (decltype(a.ExecC2R))sym("hipfftExecC2R");
        a.ExecC2C = (decltype(a.ExecC2C))sym("hipfftExecC2C");
        a.Destroy = (decltype(a.Destroy))sym("hipfftDestroy");
        return a;
    }();
    return api;
}

void fft_ok(hipfftResult r, const char *what) {
    if (r != HIPFFT_SUCCESS) throw std::runtime_error(std::string("hipFFT failure in ") + what + " (code " + std::to_string((int)r) + ")");
}

}  // namespace

Conditioner::Conditioner(int nt, int max_nrec) : nt_(nt), cap_(max_nrec) {
    const size_t npad = 2 * (size_t)nt, nf = (size_t)nt + 1;
    pad_ = DevBuf<float>(&bytes_, npad * cap_);
    spec_ = DevBuf<float2>(&bytes_, nf * cap_);
    norm_ = DevBuf<double>(&bytes_, 3 * (size_t)cap_);
}

Conditioner::~Conditioner() {
    for (auto &kv : plans_) {
        (void)fft().Destroy((hipfftHandle)kv.second.fwd);
        (void)fft().Destroy((hipfftHandle)kv.second.inv);
    }
    for (auto &kv : fk_plans_) (void)fft().Destroy((hipfftHandle)kv.second);
}

// Every kernel of the chain runs in blocks of 256 threads and is counted as one launch (launches())
template <class K, class... A> void Conditioner::launch(K kernel, dim3 grid, hipStream_t st, A... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, args...);
    launches_++;
}

bool Conditioner::idle(int nrec) const {
    if (nrec > cap_) throw std::invalid_argument("conditioning: more traces than the session was sized for");
    return nrec <= 0;
}

void Conditioner::window(hipStream_t st, float *data, int nrec, float dt, const float *win_start, const float *win_end,
                         const float *weights, float src_weight, float ratio) {
    if (idle(nrec)) return;
    launch(k_window, time_grid(nrec), st, nt_, nrec, dt, win_start, win_end, weights, src_weight, ratio, data);
}

Conditioner::Plans &Conditioner::plans_for(int nrec, hipStream_t st) {
    auto it = plans_.find(nrec);
    if (it == plans_.end()) {
        Plans p{};
        hipfftHandle f, b;
        fft_ok(fft().Plan1d(&f, 2 * nt_, HIPFFT_R2C, nrec), "hipfftPlan1d(R2C)");
        fft_ok(fft().Plan1d(&b, 2 * nt_, HIPFFT_C2R, nrec), "hipfftPlan1d(C2R)");
        p.fwd = (void *)f;
        p.inv = (void *)b;
        // Plan creation is not stream-ordered (rocFFT may build its tables with work of its own on the null stream), and the
        // session's streams are non-blocking ones that do not wait for the null stream: make sure that work is complete
        // before the plan's first use.  Once per trace count.
        if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("conditioning: hipDeviceSynchronize failed");
        it = plans_.emplace(nrec, p).first;
    }
    fft_ok(fft().SetStream((hipfftHandle)it->second.fwd, st), "hipfftSetStream");
    fft_ok(fft().SetStream((hipfftHandle)it->second.inv, st), "hipfftSetStream");
    return it->second;
}

// ---- the steps of a spectral round trip (conditioning.hpp) ----
void Conditioner::embed(hipStream_t st, const float *in, float *pad, int nrec) { launch(k_embed, pad_grid(nrec), st, nt_, nrec, in, pad); }
void Conditioner::taper_padded(hipStream_t st, float *pad, int nrec, float dt) {  // cuda_window over the PADDED length, ratio 0.01 (utilities.cu:1199-1202)
    launch(k_window, pad_grid(nrec), st, 2 * nt_, nrec, dt, nullptr, nullptr, nullptr, 1.0f, 0.01f, pad);
}
void Conditioner::forward(const Plans &pl, float *pad, float2 *spec) { fft_ok(fft().ExecR2C((hipfftHandle)pl.fwd, pad, spec), "hipfftExecR2C"), launches_++; }
void Conditioner::inverse(const Plans &pl, float2 *spec, float *pad) { fft_ok(fft().ExecC2R((hipfftHandle)pl.inv, spec, pad), "hipfftExecC2R"), launches_++; }
void Conditioner::crop(hipStream_t st, float *out, const float *pad, int nrec) { launch(k_crop, time_grid(nrec), st, nt_, nrec, out, pad, 1.0f / (float)(2 * nt_)); }

// `multiply(grid over the bins, spec_)` launches the round trip's one kernel on the spectrum
template <class M> void Conditioner::round_trip(hipStream_t st, const float *in, float *out, int nrec, M multiply) {
    const Plans &pl = plans_for(nrec, st);
    embed(st, in, pad_.get(), nrec);
    forward(pl, pad_.get(), spec_.get());
    multiply(spec_grid(nrec), spec_.get());
    inverse(pl, spec_.get(), pad_.get());
    crop(st, out, pad_.get(), nrec);
}

// bp_filter1d, utilities.cu:1115-1166
void Conditioner::bandpass(hipStream_t st, float *data, int nrec, float dt, const float filt[4]) {
    if (idle(nrec)) return;
    const float df = (float)(1.0 / (double)dt / (double)(2 * nt_));
    round_trip(st, data, data, nrec, [&](dim3 grid, float2 *spec) { launch(k_bp_filter, grid, st, nt_ + 1, nrec, df, filt[0], filt[1], filt[2], filt[3], spec); });
}

// H of the header
void Conditioner::hilbert(hipStream_t st, const float *in, float *out, int nrec) {
    if (idle(nrec)) return;
    round_trip(st, in, out, nrec, [&](dim3 grid, float2 *spec) { launch(k_hilbert_mult, grid, st, nt_ + 1, nrec, spec); });
}

// ---- the fan filter (conditioning.hpp) ----
namespace {
int fk_padded(int nrec) {  // the smallest power of two >= 2 nrec
    int P = 1;
    while (P < 2 * nrec) P *= 2;
    return P;
}
}  // namespace

void Conditioner::ensure_fk_buffers() {
    if (fk_.get()) return;
    fk_ = DevBuf<float2>(&bytes_, ((size_t)nt_ + 1) * (size_t)fk_padded(cap_));
}

void *Conditioner::fk_plan_for(int P, hipStream_t st) {
    auto it = fk_plans_.find(P);
    if (it == fk_plans_.end()) {
        hipfftHandle h;
        fft_ok(fft().Plan1d(&h, P, HIPFFT_C2C, nt_ + 1), "hipfftPlan1d(C2C)");
        // as in plans_for: plan creation is not stream-ordered
        if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("conditioning: hipDeviceSynchronize failed");
        it = fk_plans_.emplace(P, (void *)h).first;
    }
    fft_ok(fft().SetStream((hipfftHandle)it->second, st), "hipfftSetStream");
    return it->second;
}

void Conditioner::fk_filter(hipStream_t st, float *data, int nrec, float dt, double delta, const double p[4], bool reject) {
    if (idle(nrec)) return;
    if (!(delta > 0.0)) throw std::invalid_argument("conditioning: the fan filter needs a positive channel spacing");
    ensure_fk_buffers();
    const int nf = nt_ + 1, P = fk_padded(nrec);
    const size_t bins = (size_t)nf * (size_t)P;
    const Plans &pl = plans_for(nrec, st);
    hipfftHandle cc = (hipfftHandle)fk_plan_for(P, st);
    float2 *specT = fk_.get();
    embed(st, data, pad_.get(), nrec);
    forward(pl, pad_.get(), spec_.get());
    launch(k_fk_to_channels, dim3((nf + kFkTile - 1) / kFkTile, (P + kFkTile - 1) / kFkTile), st, nf, nrec, P, spec_.get(), specT);
    fft_ok(fft().ExecC2C(cc, specT, specT, HIPFFT_FORWARD), "hipfftExecC2C"), launches_++;
    launch(k_fk_gain, dim3((unsigned)((bins + 255) / 256)), st, nt_, P, 2.0 * (double)nt_ * (double)dt / ((double)P * delta), p[0], p[1], p[2], p[3], reject ? 1 : 0, specT);
    fft_ok(fft().ExecC2C(cc, specT, specT, HIPFFT_BACKWARD), "hipfftExecC2C"), launches_++;
    launch(k_fk_to_traces, dim3((nf + kFkTile - 1) / kFkTile, (nrec + kFkTile - 1) / kFkTile), st, nf, nrec, P, specT, spec_.get());
    inverse(pl, spec_.get(), pad_.get());
    launch(k_crop, time_grid(nrec), st, nt_, nrec, data, pad_.get(), (float)(1.0 / (2.0 * (double)nt_ * (double)P)));
}

void Conditioner::ensure_source_buffers(hipStream_t st) {
    if (pad2_.get()) return;
    const size_t npad = 2 * (size_t)nt_, nf = (size_t)nt_ + 1;
    pad2_ = DevBuf<float>(&bytes_, npad * cap_);
    spec2_ = DevBuf<float2>(&bytes_, nf * cap_);
    coef_ = DevBuf<float2>(&bytes_, nf);
    // ON THE CALLER'S STREAM: a plain hipMemset runs on the null stream without blocking the host, the session's streams are
    // non-blocking ones that do not wait for it, and it could land after k_matching_coef has written the coefficients -- zeroing
    // the first shot's source update or (later still) only its adjoint step: misfit right, gradient short of one shot.  That is
    // what a six-process fuzz sweep of round 3 caught once in about 15 000 draws (seed 11558: gradient 45 % off, 1.5e-6 when repeated).
    if (hipMemsetAsync(coef_.get(), 0, nf * sizeof(hipfftComplex), st) != hipSuccess) throw std::runtime_error("conditioning: hipMemsetAsync failed");
}

// source_update, utilities.cu:1170-1281
void Conditioner::source_update(hipStream_t st, const float *obs, float *syn, int nrec, float dt) {
    if (idle(nrec)) return;
    ensure_source_buffers(st);
    const int nf = nt_ + 1;
    const Plans &pl = plans_for(nrec, st);
    embed(st, obs, pad_.get(), nrec);
    embed(st, syn, pad2_.get(), nrec);
    taper_padded(st, pad_.get(), nrec, dt);
    taper_padded(st, pad2_.get(), nrec, dt);
    forward(pl, pad_.get(), spec_.get());
    forward(pl, pad2_.get(), spec2_.get());
    launch(k_matching_coef, dim3(nf), st, nf, nrec, spec_.get(), spec2_.get(), coef_.get());
    launch(k_apply_coef, spec_grid(nrec), st, nf, nrec, spec2_.get(), coef_.get(), 0);
    inverse(pl, spec2_.get(), pad2_.get());
    crop(st, syn, pad2_.get(), nrec);
}

void Conditioner::source_update_adj(hipStream_t st, float *res, int nrec, float dt) {
    if (idle(nrec)) return;
    ensure_source_buffers(st);
    const Plans &pl = plans_for(nrec, st);
    embed(st, res, pad_.get(), nrec);
    forward(pl, pad_.get(), spec_.get());
    launch(k_apply_coef, spec_grid(nrec), st, nt_ + 1, nrec, spec_.get(), coef_.get(), 1);
    inverse(pl, spec_.get(), pad_.get());
    taper_padded(st, pad_.get(), nrec, dt);
    crop(st, res, pad_.get(), nrec);
}

void Conditioner::l2_residual(hipStream_t st, const float *obs, const float *syn, float *res, int nrec, double *acc) {
    if (idle(nrec)) return;
    launch(k_l2_residual, dim3(nrec), st, nt_, nrec, obs, syn, res, acc);
}

void Conditioner::scattered_residual(hipStream_t st, const float *d, float *res, int nrec, float sign) {
    if (idle(nrec)) return;
    launch(k_scattered_residual, time_grid(nrec), st, nt_, nrec, d, res, sign);
}

void Conditioner::cross_residual(hipStream_t st, const float *obs, const float *syn, float *res, int nrec, const float *weights,
                                 float src_weight, double *acc) {
    if (idle(nrec)) return;
    double *n_oo = norm_.get(), *n_ss = n_oo + cap_, *n_os = n_oo + 2 * (size_t)cap_;
    launch(k_normfact, dim3(nrec), st, nt_, obs, obs, n_oo);
    launch(k_normfact, dim3(nrec), st, nt_, syn, syn, n_ss);
    launch(k_normfact, dim3(nrec), st, nt_, obs, syn, n_os);
    launch(k_cross_misfit, dim3(1), st, nrec, n_os, n_oo, n_ss, weights, src_weight, acc);
    launch(k_cross_adjoint, time_grid(nrec), st, nt_, nrec, n_oo, n_ss, n_os, obs, syn, res, weights, src_weight);
}

void Conditioner::ensure_envelope_buffers() {
    if (env_.get()) return;
    env_ = DevBuf<float>(&bytes_, 3 * (size_t)nt_ * cap_);
    env_sum_ = DevBuf<double>(&bytes_, (size_t)cap_);
}

void Conditioner::envelope_residual(hipStream_t st, const float *obs, const float *syn, float *res, int nrec, double *acc) {
    if (idle(nrec)) return;
    ensure_envelope_buffers();
    const size_t g = (size_t)nt_ * cap_;
    float *hd = env_.get(), *hs = hd + g, *b = hd + 2 * g;
    launch(k_env_diff, time_grid(nrec), st, nt_, nrec, obs, syn, hd);
    hilbert(st, hd, hd, nrec);  // H (obs - syn), in place (the transform reads its input into the padded buffer first)
    hilbert(st, syn, hs, nrec);
    launch(k_env_residual, dim3(nrec), st, nt_, obs, hd, syn, hs, res, b, env_sum_.get());
    launch(k_env_sum, dim3(1), st, nrec, env_sum_.get(), acc);
    hilbert(st, b, b, nrec);
    launch(k_env_combine, time_grid(nrec), st, nt_, nrec, res, b, 1.0f);
}

void Conditioner::ensure_w2_buffers() {
    if (w2_.get()) return;
    w2_ = DevBuf<double>(&bytes_, kW2Planes * (size_t)nt_ * cap_);
    w2_sum_ = DevBuf<double>(&bytes_, (size_t)cap_);
}

void Conditioner::w2_residual(hipStream_t st, const float *obs, const float *syn, float *res, int nrec, const float *weights, float src_weight,
                              float dt, double beta, double *acc) {
    if (idle(nrec)) return;
    ensure_w2_buffers();
    launch_w2_trace(st, nt_, nrec, obs, syn, res, weights, src_weight, dt, beta, w2_.get(), (size_t)nt_ * cap_, w2_sum_.get());
    launches_++;
    launch(k_env_sum, dim3(1), st, nrec, w2_sum_.get(), acc);  // the traces in a fixed order
}

void Conditioner::ensure_robust_buffers() {
    if (robust_scale_.get()) return;
    robust_scale_ = DevBuf<float>(&bytes_, (size_t)cap_);
    robust_sum_ = DevBuf<double>(&bytes_, (size_t)cap_);
}

void Conditioner::robust_residual(hipStream_t st, const float *obs, const float *syn, float *res, int nrec, int kind, double delta, double quantile,
                                  double *acc) {
    if (idle(nrec)) return;
    ensure_robust_buffers();
    launch_robust_trace(st, nt_, nrec, obs, syn, nullptr, res, kind, delta, robust_rank(nt_, quantile), 1.0f, robust_scale_.get(), robust_sum_.get());
    launches_++;
    launch(k_env_sum, dim3(1), st, nrec, robust_sum_.get(), acc);  // the traces in a fixed order
}

void Conditioner::robust_scattered(hipStream_t st, const float *obs, const float *syn_bg, const float *d, float *res, int nrec, int kind,
                                   double delta, double quantile, float sign) {
    if (idle(nrec)) return;
    ensure_robust_buffers();
    launch_robust_trace(st, nt_, nrec, obs, syn_bg, d, res, kind, delta, robust_rank(nt_, quantile), sign, robust_scale_.get(), robust_sum_.get());
    launches_++;
}

void Conditioner::envelope_scattered(hipStream_t st, const float *syn, const float *d, float *res, int nrec, float sign) {
    if (idle(nrec)) return;
    ensure_envelope_buffers();
    const size_t g = (size_t)nt_ * cap_;
    float *hd = env_.get(), *hs = hd + g, *b = hd + 2 * g;
    hilbert(st, d, hd, nrec);
    hilbert(st, syn, hs, nrec);
    launch(k_env_linear, time_grid(nrec), st, nt_, nrec, syn, hs, d, hd, res, b);
    hilbert(st, b, b, nrec);
    launch(k_env_combine, time_grid(nrec), st, nt_, nrec, res, b, sign);
}

}  // namespace sepfwi
