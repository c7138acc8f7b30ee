// conditioning.hpp -- data-conditioning chain of the misfit (conditioning.hip): windows, band-pass (hipFFT), normalised
// cross-correlation misfit, envelope misfit, trace-wise W2 misfit, robust (Huber / Cauchy) misfits, f-k fan filter.  All gathers are [rec][nt] float32 device arrays.
#pragma once
#include <hip/hip_runtime.h>

#include <map>

#include "device_alloc.hpp"

namespace sepfwi {

class Conditioner {
  public:
    Conditioner(int nt, int max_nrec);
    ~Conditioner();
    Conditioner(const Conditioner &) = delete;
    Conditioner &operator=(const Conditioner &) = delete;

    // cuda_window (utilities.cu:787-884): win_start == nullptr -> one end taper for all traces; else per-trace windows
    // [win_start, win_end] in seconds and amplitude weights[r] * src_weight.  ratio: libCUFD.cu:63 (0.005).
    void window(hipStream_t st, float *data, int nrec, float dt, const float *win_start, const float *win_end, const float *weights,
                float src_weight, float ratio);
    // bp_filter1d (utilities.cu:1115-1166): zero-phase sin^2 / cos^2 band-pass with corners filt[0..3] Hz, in place
    void bandpass(hipStream_t st, float *data, int nrec, float dt, const float filt[4]);
    // gpuMinus + cuda_cal_objective (utilities.cu:154-205): res = obs - syn (first sample zeroed), *acc += sum res^2
    void l2_residual(hipStream_t st, const float *obs, const float *syn, float *res, int nrec, double *acc);
    // what l2_residual leaves in res for observed data syn - d: res = -d (first sample zeroed); no misfit is accumulated
    // (sign = 1: +Z d, what sepfwi_data_gn hands out)
    void scattered_residual(hipStream_t st, const float *d, float *res, int nrec, float sign = -1.0f);
    // ---- envelope misfit (parameter key if_envelope_misfit) ----
    // The discrete Hilbert transform H of every trace: zero-pad to 2 nt, R2C, bin k times -i for 0 < k < nt and times 0 for k = 0 and
    // k = nt, C2R, 1 / (2 nt), crop -- the padding, plans and buffers of bandpass.  H^T = -H exactly.  in == out is allowed.
    void hilbert(hipStream_t st, const float *in, float *out, int nrec);
    // Squared envelope e(x) = x^2 + (H x)^2, pointwise.  rho = Z (e(obs) - e(syn)), Z the zeroing of sample 0; *acc += sum rho^2 (double,
    // a fixed order of additions: no atomics); res = D^T rho = 2 [syn rho - H((H syn) rho)], which is -d(1/2 |rho|^2)/d syn -- the sign of
    // l2_residual.  ARITHMETIC: e, rho and res are float32 and scale with the second and third power of the data; nothing rescales
    // them.  Data whose squares or cubes leave the float32 range must be scaled by the survey's weights / src_weight (if_win).
    // obs, syn and res must be three different gathers.
    void envelope_residual(hipStream_t st, const float *obs, const float *syn, float *res, int nrec, double *acc);
    // The linearised twin at the background syn: res = sign D^T Z D d with D = 2 [diag(syn) + diag(H syn) H].  sign = -1: what
    // envelope_residual leaves for observed data whose envelope is e(syn) - D d (the Gauss-Newton product); no misfit.
    void envelope_scattered(hipStream_t st, const float *syn, const float *d, float *res, int nrec, float sign = -1.0f);
    // cuda_find_normfact x3 + cuda_normal_misfit + cuda_normal_adjoint_source (utilities.cu:1010-1111):
    // *acc += -2 sum_r <obs,syn>_r / (|obs|_r |syn|_r) w_r ; res = the adjoint source.  weights may be null (all ones).
    void cross_residual(hipStream_t st, const float *obs, const float *syn, float *res, int nrec, const float *weights, float src_weight,
                        double *acc);
    // ---- trace-wise quadratic Wasserstein misfit (parameter key if_w2_misfit; w2_misfit.hpp holds the definition) ----
    // *acc += sum_r w_r W_r (the driver halves the total), W_r the squared transport distance between the softplus densities of syn and obs
    // in time; res = -1/2 w_r dW_r / d syn, the sign of l2_residual.  w_r = weights[r] * src_weight, or 1 where weights is null (the rule of
    // cross_residual).  Double from the densities onwards, res rounded once; no atomics.  obs, syn and res: three different gathers.
    void w2_residual(hipStream_t st, const float *obs, const float *syn, float *res, int nrec, const float *weights, float src_weight, float dt,
                     double beta, double *acc);
    // ---- robust misfits (parameter keys robust_misfit / robust_delta / robust_quantile; robust_misfit.hpp holds the definition) ----
    // kind: kRobustHuber or kRobustCauchy.  Per trace A = the order statistic floor(quantile (nt - 2)) of |obs| over samples 1 ... nt - 1 (an
    // exact radix select), the threshold delta A; res = psi (sample 0 zeroed), the sign of l2_residual; *acc += 2 sum phi, the traces in a fixed
    // order.  Double from the residual onwards, res rounded once; no floating-point atomics.  obs, syn and res: three different gathers.
    void robust_residual(hipStream_t st, const float *obs, const float *syn, float *res, int nrec, int kind, double delta, double quantile,
                         double *acc);
    // The linearised twin: res = sign Z w Z d with the IRLS weight w of (obs, the background syn_bg), 0 on dead traces.  sign = -1: what
    // robust_residual leaves, to first order in the weights' own terms, for observed data syn_bg - d (the Gauss-Newton product); no misfit.
    void robust_scattered(hipStream_t st, const float *obs, const float *syn_bg, const float *d, float *res, int nrec, int kind, double delta,
                          double quantile, float sign = -1.0f);
    // ---- apparent-slowness (f-k) fan filter across the channels of one shot (parameter keys fk_slowness / fk_mode) ----
    // In place on the [nrec][nt] gather: zero-pad to [P][2 nt], P the smallest power of two >= 2 nrec; forward DFT along both axes (e^{-i...}:
    // the R2C of bandpass along time, rows j = 0 ... nt, f_j = j / (2 nt dt); a C2C of length P along the channels, k_m = m / (P delta) for
    // m <= P / 2, else (m - P) / (P delta)); every bin times the real gain G of its apparent slowness p = -k / f (p > 0: an event that arrives
    // later at higher channel indices; at f = 0: p = 0 for k = 0, G's value at infinity otherwise); both inverse transforms, 1 / (2 nt P), crop.
    // G = T in pass mode, 1 - T with `reject`; T(p) = 0 outside (p[0], p[3]), 1 on [p[1], p[2]], sin^2 / cos^2 ramps between.  On the time-Nyquist
    // row j = nt and the wavenumber-Nyquist column m = P / 2 the gain is (T(p) + T(-p)) / 2: the half-spectrum computation then equals the
    // full complex one and the operator is exactly symmetric (its own transpose), like bandpass.  delta: the channel spacing [m].
    // The gain is evaluated in the kernel in double (no table); float32 transforms, no atomics: the same input gives the same bits.
    // Between the time and channel transforms the spectrum is transposed ([nrec][nt + 1] <-> [nt + 1][P], LDS tiles), so that both run on
    // contiguous batches; the rows nrec ... P - 1 of the padding are written by the transposition and never transformed along time.
    void fk_filter(hipStream_t st, float *data, int nrec, float dt, double delta, const double p[4], bool reject);
    // the transposed spectrum [nt + 1][Pcap] float2, Pcap the smallest power of two >= 2 cap, allocated on first use: a session whose file does
    // not set the key never holds it.  8 (nt + 1) Pcap bytes: 131 MB at 1980 channels x 4000 samples (Pcap = 4096), beside the 127 MB of the
    // padded gather and its spectrum that bandpass holds anyway (hipFFT's own work areas are not counted).
    void ensure_fk_buffers();
    // source_update (utilities.cu:1170-1281, cuda_spectrum_update :905-977): the source-signature update as a matching filter.
    // Both gathers zero-padded to 2 nt and end-tapered over the padded length (ratio 0.01); per frequency one coefficient
    // coef(f) = sum_r conj(C_r) O_r / (sum_r |C_r|^2 + 1e-6), kept for the adjoint step; the synthetic spectra are multiplied by
    // it, transformed back, cropped.  `syn` is updated in place, `obs` is only read.
    void source_update(hipStream_t st, const float *obs, float *syn, int nrec, float dt);
    // transpose of the map syn -> updated syn at the coefficients of the last source_update: pad, FFT, conj(coef), inverse FFT,
    // end taper of the padded length, crop.  (Conscious fix of source_update_adj, utilities.cu:1283-1325: oracle/oracle.py.)
    void source_update_adj(hipStream_t st, float *res, int nrec, float dt);
    // the second padded gather / spectrum and the coefficients of the source update, allocated (and the coefficients zeroed on `st`)
    // once; the session calls it up-front when the parameter file sets if_src_update, so that no shot pays an allocation inside
    // its time loop
    void ensure_source_buffers(hipStream_t st);
    // three [cap][nt] scratch gathers (H obs or H d, H syn, (H syn) rho) and the per-trace sums of the envelope misfit, allocated on
    // first use: a session whose file does not set the key never holds them
    void ensure_envelope_buffers();
    // five [cap][nt] double scratch planes (the CDFs, the densities, c) and the per-trace w_r W_r of the W2 misfit, allocated on first use
    void ensure_w2_buffers();
    // the per-trace scale A and sums 2 sum phi of the robust misfits, allocated on first use
    void ensure_robust_buffers();
    long long device_bytes() const { return bytes_; }  // what the buffers below hold
    // What the methods above have issued so far: one per kernel launch and one per hipFFT exec (a plan's creation is none).  Per gather
    // with channels:
    //   window, l2_residual, scattered_residual   1
    //   bandpass, hilbert                         5   embed, R2C, the spectrum's multiplier, C2R, crop
    //   cross_residual                            5   three norms, misfit, adjoint source
    //   source_update                            10   2 embeds, 2 tapers, 2 R2C, coefficients, their product, C2R, crop
    //   source_update_adj                         6   embed, R2C, conj(coef), C2R, taper, crop
    //   envelope_residual                        19   difference, 2 hilbert, residual, sum, hilbert, combination
    //   envelope_scattered                       17   2 hilbert, linearised residual, hilbert, combination
    //   w2_residual                               2   the traces (one block each), their sum
    //   robust_residual                           2   the traces (one block each: select, then residual), their sum
    //   robust_scattered                          1   the traces (select, then the weighted product)
    //   fk_filter                                 9   embed, R2C, transposition, C2C, the gain, C2C, transposition, C2R, crop
    long long launches() const { return launches_; }

  private:
    struct Plans {
        void *fwd, *inv;  // hipfftHandle
    };
    Plans &plans_for(int nrec, hipStream_t st);
    void *fk_plan_for(int P, hipStream_t st);  // the C2C plan of nt + 1 contiguous transforms of length P, made as plans_for makes its plans
    // true: no traces, nothing to do.  Throws for a gather of more traces than the work space holds.
    bool idle(int nrec) const;
    template <class K, class... A> void launch(K kernel, dim3 grid, hipStream_t st, A... args);
    dim3 time_grid(int nrec) const { return dim3((nt_ + 255) / 256, nrec); }      // one thread per sample of [nrec][nt]
    dim3 pad_grid(int nrec) const { return dim3((2 * nt_ + 255) / 256, nrec); }   // ... of the padded [nrec][2 nt]
    dim3 spec_grid(int nrec) const { return dim3((nt_ + 1 + 255) / 256, nrec); }  // ... per bin of the spectra [nrec][nt + 1]
    // The spectral round trip of bandpass and hilbert: `in` zero-padded to 2 nt in pad_, R2C into spec_, `multiply` on the spectrum, C2R,
    // crop with the 1 / (2 nt) of the unnormalised inverse transform into `out` (in == out is allowed: `in` is read into pad_ first).
    template <class M> void round_trip(hipStream_t st, const float *in, float *out, int nrec, M multiply);
    // Its steps; the source update composes them itself (two gathers, pad_ / spec_ and pad2_ / spec2_, and the end taper of the padded
    // length, ratio 0.01).  `pl` is plans_for(nrec, st) of the same call.
    void embed(hipStream_t st, const float *in, float *pad, int nrec);
    void taper_padded(hipStream_t st, float *pad, int nrec, float dt);
    void forward(const Plans &pl, float *pad, float2 *spec);
    void inverse(const Plans &pl, float2 *spec, float *pad);
    void crop(hipStream_t st, float *out, const float *pad, int nrec);
    int nt_, cap_;
    long long bytes_ = 0, launches_ = 0;
    DevBuf<float> pad_, pad2_;
    DevBuf<double> norm_;          // the three per-trace norms of the cross-correlation misfit, 3 x [cap]
    DevBuf<float2> spec_;          // hipfftComplex [cap][nt + 1]
    DevBuf<float2> spec2_, coef_;  // second padded gather / spectrum and the nt + 1 matching-filter coefficients (source update)
    DevBuf<float> env_;            // envelope misfit: 3 x [cap][nt]
    DevBuf<double> env_sum_;       // ... and sum rho^2 per trace
    DevBuf<double> w2_, w2_sum_;   // W2 misfit: kW2Planes x [cap][nt], and w_r W_r per trace
    DevBuf<float> robust_scale_;   // robust misfits: A per trace
    DevBuf<double> robust_sum_;    // ... and 2 sum phi per trace
    DevBuf<float2> fk_;            // fan filter: the transposed spectrum [nt + 1][Pcap]
    std::map<int, Plans> plans_;  // by number of traces
    std::map<int, void *> fk_plans_;  // by padded channel count P
};

}  // namespace sepfwi
