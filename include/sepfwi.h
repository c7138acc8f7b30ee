/*
 * sepfwi.h -- C ABI of libsepfwi.so: MI355X-native 2-D elastic staggered-grid forward/adjoint
 * propagator (velocity-stress, C-PML, boundary-saving reconstruction, DAS axial-strain receivers).
 *
 * This is the drop-in boundary for the hot path of seisfwi/SEP-2023 "TorchFWI-DAS".  Every entry
 * point names the reference interface it replaces (paths relative to
 * DAS_Waveform_Inversion/Ops/FWI/ in the reference repository).  Plain pointers and sizes only; no
 * torch types, no C++ types.  All functions return 0 on success and a negative SEPFWI_E* code on
 * failure; sepfwi_last_error() then holds a message (the reference printf()s and exit(1)s instead:
 * Src/utilities.h:28-36, Src/utilities.cu:12-16,237-240).
 *
 * Pointer arguments documented as "host or device" may be either: transfers use
 * hipMemcpyDefault, so a torch CPU tensor's data_ptr and a torch HIP tensor's data_ptr both work.
 */
#ifndef SEPFWI_H_
#define SEPFWI_H_

#ifdef __cplusplus
extern "C" {
#endif

#define SEPFWI_OK 0
#define SEPFWI_EINVAL (-1)   /* bad argument / inconsistent sizes                         */
#define SEPFWI_EIO (-2)      /* parameter, survey or data file missing / unreadable       */
#define SEPFWI_ECOURANT (-3) /* Courant number > 1            (Src/utilities.cu:225-241)  */
#define SEPFWI_EHIP (-4)     /* HIP runtime error (no device, out of memory, launch fault)*/
#define SEPFWI_EJSON (-5)    /* malformed parameter / survey JSON                         */

/* calc_id values (Src/libCUFD.cu:22-25, Src/Parameter.cpp:125-137) */
#define SEPFWI_CALC_MISFIT 0   /* forward + residual -> misfit                      */
#define SEPFWI_CALC_GRADIENT 1 /* + boundary saving, adjoint, gradients             */
#define SEPFWI_CALC_OBSERVE 2  /* forward only, write Shot_{pr,vx,vz,ett}{id}.bin   */
/* Extension (no counterpart in the reference): forward only, and the axial-strain gather of every shot goes straight into the
 * session's HBM store of observed data -- what SEPFWI_CALC_OBSERVE followed by reading Shot_ett{id}.bin back would leave there,
 * bit for bit, without the four files per shot (synthetic studies, benchmarks).  No other output. */
#define SEPFWI_CALC_OBSERVE_TO_STORE 3

/* Message of the last failure on the calling thread (never NULL). */
const char *sepfwi_last_error(void);

/* Library version, e.g. 100 = 0.1.0 */
int sepfwi_version(void);

/* Number of visible HIP devices, or a negative error code. */
int sepfwi_device_count(void);

/*
 * Replaces:  extern "C" void cufd(float *misfit, float *grad_Lambda, float *grad_Mu,
 *                float *grad_Den, float *grad_stf, const float *Lambda, const float *Mu,
 *                const float *Den, const float *stf, int calc_id, const int gpu_id,
 *                const int group_size, const int *shot_ids, const string para_fname)
 *            Src/libCUFD.h:6-10, Src/libCUFD.cu:32-820
 * called from Src/Torch_Fwi.cpp:31,86,132.  Same argument order and meaning; std::string became
 * const char*, void became an error code.
 *
 *   Lambda, Mu   [MPa], Den [kg/m^3]: (nz, nx) row-major float32, nz/nx the padded sizes of the
 *                parameter file (FWI_ops.py:124-127).  Host or device.
 *   stf          (nSrc, nSteps) row-major; row shot_ids[i] is shot i's source (Src/Src_Rec.cu:9,132).
 *                Host or device.
 *   shot_ids     group_size ints, host.
 *   misfit       1 float (calc_id 0,1): 0.5 * sum over shots of sum r_ett^2 (libCUFD.cu:427,776).
 *   grad_Lambda, grad_Mu, grad_Den   (nz, nx) row-major, OVERWRITTEN with this call's sum over its
 *                shots (calc_id 1).  Gradients are w.r.t. MPa for Lambda/Mu.  Host or device.
 *   grad_stf     (group_size, nSteps): row i = shot_ids[i] (local position, libCUFD.cu:671-673).
 *   para_fname   one-line JSON written by fwi_utils.paraGen (fwi_utils.py:46-83); names the survey
 *                JSON (fwi_utils.py:87-124) and the data directory holding
 *                Shot_{pr,vx,vz,ett}{id}.bin, float32 [nrec][nSteps] (libCUFD.cu:216-223,755-769).
 *                One optional key beyond the reference's schema: "das_fiber": "horizontal" (default: ett = exx,
 *                recording_exx / res_injection_exx) or "vertical" (ett = ezz, recording_ezz / res_injection_ezz,
 *                Src/utilities.cu:620-641, which the reference reaches only through a source edit).  Further optional keys
 *                (INTEGRATION.md): "obs_pack_fname" -- one packed file of the survey's observed axial-strain gathers instead
 *                of four files per shot; "if_win", "filter", "if_cross_misfit", "if_src_update" -- the data-conditioning
 *                chain of Src/utilities.cu:733-1325, dormant in the reference's driver, live here for the axial-strain gathers;
 *                "das_gauge_length" [m] -- every channel records the mean axial strain over a gauge of G = L / dx cells along a
 *                horizontal fibre (L / dz along a vertical one; directional channels take the das_fiber axis), its adjoint
 *                source the exact transpose.  L must be a whole multiple of the spacing (SEPFWI_EJSON otherwise), every
 *                member cell of a gauge must lie where a channel may (SEPFWI_EINVAL).  Absent or G = 1: the one-cell channel.
 *                "misfit_w_ett" (default 1), "misfit_w_vx" (0), "misfit_w_vz" (0) -- weights of the axial-strain, vx and vz residuals:
 *                  misfit = 0.5 sum_shots ( w_ett sum r_ett^2 + w_vx sum r_vx^2 + w_vz sum r_vz^2 ),  r_c = obs_c - syn_c
 *                (time sample 0 forced to 0); vx / vz are sampled at the channel's own cell, the adjoint source of component c is
 *                w_c r_c added to vx_adj / vz_adj of that cell where the strain residual enters (Src/libCUFD.cu:600-607; the
 *                reference ships res_injection_vx / _vz, Src/utilities.cu:656-689, and never launches them: an extension that no
 *                reference run pins).  Each weight finite and >= 0, not all zero (SEPFWI_EJSON).  Observed data of a component with a
 *                weight come from Shot_{vx,vz,ett}{id}.bin, sepfwi_set_observed_component or calc_id 3; a component with weight 0
 *                is never read.  misfit_w_vx / misfit_w_vz > 0 with "obs_pack_fname", and any weights other than (1, 0, 0) with a
 *                live conditioning key, are refused (SEPFWI_EINVAL).  Absent or (1, 0, 0): bit for bit the axial-strain misfit.
 *                "if_envelope_misfit": true (an extension that no reference run pins) -- the envelope misfit, for data whose low
 *                frequencies are missing and whose waveform misfit cycle-skips.  With o = C obs, s = C syn (C as under
 *                sepfwi_condition below), H the discrete Hilbert transform (zero-pad to 2 nSteps, real FFT, bin k times -i for
 *                0 < k < nSteps and times 0 for k = 0 and k = nSteps, inverse FFT, crop: H^T = -H exactly) and the SQUARED envelope
 *                e(x) = x^2 + (H x)^2:
 *                  misfit = 0.5 sum_shots |rho|^2,  rho = Z (e(o) - e(s)),  Z the zeroing of time sample 0;
 *                  adjoint source = -d misfit / d syn = C^T D^T rho,  D^T rho = 2 [ s rho - H((H s) rho) ].
 *                A polynomial in the data: no division, no floor, every derivative exact.  ARITHMETIC: e, rho and the adjoint
 *                source are float32 and scale with the second and third power of the data; nothing rescales them -- the survey's
 *                "weights" / "src_weight" (with if_win) are the user's handle on the amplitudes.  A live conditioning key: it
 *                composes with if_win and filter; with "conditioning": "reference" it is parsed and ignored like the other four.
 *                Refused (SEPFWI_EINVAL): together with if_cross_misfit, with if_src_update, or with weights other than (1, 0, 0).
 *                Absent or false: every launch, allocation and bit as before.
 *                "if_w2_misfit": true, "w2_beta": b (an extension that no reference run pins) -- the trace-wise quadratic Wasserstein
 *                (optimal-transport) misfit of Engquist & Froese 2014 and Yang et al. 2018, the other remedy for cycle-skipped data.
 *                Per trace, o = C obs, s = C syn with n = nSteps samples, t_i = i dt, i = 1 ... n - 1 (sample 0 carries no mass):
 *                  A = max |o| over the trace (A == 0: a dead trace, misfit 0 and adjoint source 0);
 *                  q(x) = softplus(b x / A);  f = q(s) / sum q(s),  g = q(o) / sum q(o);  F, G their prefix sums (G_0 = 0);
 *                  j(i) the first j >= 1 with G_j >= F_i;  T_i = t_{j-1} + dt (F_i - G_{j-1}) / g_j;  W = sum_i f_i (t_i - T_i)^2;
 *                  misfit = 0.5 sum_shots sum_r w_r W_r,  w_r = weights[r] * src_weight under if_win, else 1 (the window's amplitude
 *                  weight cancels in the densities, so the trace weight is explicit -- the rule of if_cross_misfit);
 *                  adjoint source = -d misfit / d syn = -0.5 C^T w dW / ds, the exact derivative at fixed j (csrc/w2_misfit.hpp).
 *                The scale A comes from the observed trace alone: a constant under differentiation, and a synthetic of the wrong
 *                amplitude is still penalised.  w2_beta in (0, 16], default 3 (the smallest whole value at which the misfit of a
 *                two-arrival 15 Hz Ricker trace grows monotonically over 2.25 periods of shift).  ARITHMETIC: the map amplifies a
 *                relative 1e-7 of its inputs to 1e-5 of the adjoint source, so everything from q onwards is double and the adjoint
 *                source is rounded to float32 once; no atomics, the same input gives the same bits.  A live conditioning key: it
 *                composes with if_win and filter; with "conditioning": "reference" it is parsed and ignored.  Refused
 *                (SEPFWI_EINVAL): together with if_cross_misfit, if_envelope_misfit, if_src_update or weights other than (1, 0, 0);
 *                a w2_beta outside (0, 16].  Absent or false: every launch, allocation and bit as before.
 *                "robust_misfit": "huber" | "cauchy", "robust_delta": c, "robust_quantile": q (an extension that no reference run pins) --
 *                a robust misfit for data with spikes, dropouts and fading channels (Guitton & Symes 2003; Aravkin et al. 2011).  Per
 *                trace, o = C obs, s = C syn, the n = nSteps - 1 live samples i = 1 ... nSteps - 1 (csrc/robust_misfit.hpp):
 *                  A = the order statistic of index floor(q (n - 1)), from the smallest, of |o_i| -- exact, no interpolation
 *                  (A == 0: a dead trace, misfit 0 and adjoint source 0);  delta = c A;  r = o - s;  u = r / delta;
 *                  huber:  phi = delta^2 u^2 / 2 for |u| <= 1, else delta^2 (|u| - 1/2);  w = min(1, 1 / |u|)
 *                  cauchy: phi = delta^2 / 2 log1p(u^2);  w = 1 / (1 + u^2)
 *                  misfit = sum_shots sum_r sum_i phi;  adjoint source = -d misfit / d syn = C^T Z (r w).
 *                The scale A comes from the observed trace alone: a constant under differentiation.  The Gauss-Newton products use the
 *                IRLS form C^T Z diag(w) Z C with w at the background -- symmetric, non-negative, the L2 operator where |r| <= delta
 *                (huber); not the true Hessian (0 on huber's outliers, indefinite for cauchy).  robust_delta is REQUIRED with the key
 *                (finite, > 0; no default: it depends on the data's noise); robust_quantile in (0, 1], default 0.9 (spikes and dropouts
 *                fill far less than a tenth of a trace, a windowed arrival normally more; a trace whose signal fills less needs if_win
 *                or a larger value, else A falls to the noise floor and the trace is treated as L1).  Under if_win WITHOUT a filter the
 *                samples outside a trace's window are exact zeros and count among the n: a trace whose window covers less than 1 - q of
 *                the record has A = 0 and is dead (three random draws of tests/test_gpu_robust_fuzz.py under if_win alone, windows of
 *                3 ... 10 % of the record at the median: 211 of 212, 32 of 66 and 3 of 5 traces dead at q = 0.9, 38, 10 and 1 at 0.99,
 *                none at 1.0).  ARITHMETIC: double from r onwards,
 *                the adjoint source rounded to float32 once; no floating-point atomics, the same input gives the same bits.  A live
 *                conditioning key: it composes with if_win and filter; with "conditioning": "reference" it is parsed, validated and
 *                ignored.  Refused (SEPFWI_EINVAL): any other kind; the key without robust_delta; robust_delta or robust_quantile without
 *                the key or out of range; together with if_cross_misfit, if_envelope_misfit, if_w2_misfit, if_src_update or weights
 *                other than (1, 0, 0).  Absent: every launch, allocation and bit as before.
 *                "fk_slowness": [p1, p2, p3, p4] (s/m), "fk_mode": "pass" | "reject" (default "pass") (an extension that no reference run
 *                pins) -- the apparent-slowness (f-k) fan filter across the channels of a shot, the third stage of the conditioning
 *                chain: C = FK . band-pass . window, C^T = window . band-pass . FK (sepfwi_condition below).  On a shot's [nrec][nSteps]
 *                gather: zero-pad to [P][2 nSteps], P the smallest power of two >= 2 nrec; forward DFT along both axes; every bin
 *                times the real gain G of its slowness p = -k / f (p > 0: an event that arrives later at higher channel indices; at
 *                f = 0: p = 0 for k = 0, infinite otherwise); inverse transforms, crop.  G = T (pass) or 1 - T (reject), T(p) = 0 outside
 *                (p1, p4), 1 on [p2, p3], sin^2 / cos^2 ramps between; on the time-Nyquist row and the wavenumber-Nyquist column
 *                (T(p) + T(-p)) / 2, which makes the operator exactly symmetric.  The channel spacing comes from the survey: every
 *                shot's channels must lie on one straight, equally spaced line in channel order ((z_rec, x_rec) steps all equal and
 *                not (0, 0); spacing sqrt((sz dz)^2 + (sx dx)^2), shot by shot); a shot without channels is idle.  float32
 *                transforms, the gain in double, no atomics: the same input gives the same bits.  A live conditioning key: alone it
 *                switches the window stage to its end taper; it composes with if_win, filter and every misfit kind (they see C obs
 *                and C syn alone); with "conditioning": "reference" it is parsed, validated and ignored.  Refused (SEPFWI_EINVAL):
 *                fk_slowness that is not four finite numbers p1 < p2 <= p3 < p4; another fk_mode; fk_mode without fk_slowness;
 *                together with weights other than (1, 0, 0); at session creation a shot with exactly one channel, a channel step
 *                that changes or a zero step (the message names the shot and the channel).  Absent: every launch, allocation and
 *                bit as before.
 *
 * Unlike the reference, device state (fields, PML profiles, boundary buffers, observed data) is kept
 * in a per-(para_fname, gpu_id) session between calls; sepfwi_release_all() frees it.
 */
int sepfwi_cufd(float *misfit, float *grad_Lambda, float *grad_Mu, float *grad_Den,
                float *grad_stf, const float *Lambda, const float *Mu, const float *Den,
                const float *stf, int calc_id, int gpu_id, int group_size, const int *shot_ids,
                const char *para_fname);

/* Same as sepfwi_cufd, but all launches go to `hip_stream` (a hipStream_t, may be NULL), and with `async` != 0 and every output
 * pointer (misfit, gradients) a device pointer the call does not end with a device synchronisation: the outputs are complete when the
 * work queued on the stream is -- the caller synchronises its stream before reading them
 * (tests/test_gpu_parity.py::test_c_abi_on_a_caller_stream_without_final_synchronisation).  `async` is NOT a promise that the host
 * returns early: the call synchronises the stream internally between the passes of a shot (to form the misfit on the host side of
 * the forward pass, and once per backward pass to learn whether the persistent loop's grid started -- a pass that does not start must
 * be re-issued as per-step launches), so it returns when all but the final gradient kernels have run. */
int sepfwi_cufd_stream(float *misfit, float *grad_Lambda, float *grad_Mu, float *grad_Den,
                       float *grad_stf, const float *Lambda, const float *Mu, const float *Den,
                       const float *stf, int calc_id, int gpu_id, int group_size,
                       const int *shot_ids, const char *para_fname, void *hip_stream, int async);

/* Frees every cached session (device memory, cached observed data) of this process. */
void sepfwi_release_all(void);

/*
 * Observed axial-strain data of one shot from memory instead of Shot_ett{id}.bin (the reference re-reads
 * four files per shot on every call, Src/libCUFD.cu:216-223).  `ett` is [nrec][nSteps] float32 like the file, host or
 * device pointer; the session keeps a time-major copy in HBM and uses it for every later misfit / gradient call of that
 * shot until sepfwi_invalidate_observed() or sepfwi_release_all().  No file is needed for shots set this way.
 */
int sepfwi_set_observed(const char *para_fname, int gpu_id, int shot_id, const float *ett, int nrec, int nSteps);

/*
 * The same for one component of a joint misfit (parameter keys misfit_w_*): comp 1 (vx), 2 (vz) or 3 (ett, what
 * sepfwi_set_observed means) -- the reference's component order, Shot_{vx,vz,ett}{id}.bin.  Any other comp: SEPFWI_EINVAL.
 */
int sepfwi_set_observed_component(const char *para_fname, int gpu_id, int shot_id, int comp, const float *data, int nrec, int nSteps);

/*
 * The unweighted parts 0.5 sum_shots sum r_c^2 of the last misfit or gradient call of (para_fname, gpu_id), for (vx, vz, ett) -- what
 * a user needs to choose the weights.  The entry of a component with weight 0 is 0.  Per process, not all-reduced.  SEPFWI_EINVAL
 * without a session.
 */
int sepfwi_get_misfit_parts(const char *para_fname, int gpu_id, double parts[3]);

/*
 * Extension (no counterpart in the reference; no reference run pins it): the diagonal pseudo-Hessian of Shin et al. (2001), i.e. the
 * source-side illumination per parameter, accumulated from the forward wavefield of a misfit or gradient call -- a preconditioner for
 * the three gradients, not a Hessian.  On every forward step it with it % every == 0 (weight `every`), for the cells of the imaging
 * condition (nPml <= z <= nz - nPad - 1 - nPml, nPml <= x <= nx - 1 - nPml), summed over the shots of the call:
 *   hLambda = 2 (1e6 dt)^2 sum (a + b)^2,   hMu = (1e6 dt)^2 sum (4 a^2 + 4 b^2 + s^2),   hDen = dt^2 sum ((ba^2/2 Fz)^2 + (bb^2/2 Fx)^2)
 * with a = dvz/dz, b = dvx/dx, s = dvx/dz + dvz/dx of the velocities at the start of the step, Fz = dszz/dz + dsxz/dx and
 * Fx = dsxz/dz + dsxx/dx of the stresses after the step's stress update and source add, ba / bb the buoyancy averages of the cell:
 * the squared forward-side factors of the three imaging conditions, each at its own staggered point (the gathers of the gradient
 * finalisation are left out on purpose).  Zero elsewhere.  Same units as the squared gradients (MPa, kg/m^3).
 */
/* every >= 1 arms the session of (para_fname, gpu_id), creating it as sepfwi_set_observed does;
   0 disarms; < 0: SEPFWI_EINVAL before anything else is touched.  Only calc_id 0 and 1 accumulate; a call that is not armed issues
   exactly the launches it issued before.  The result is that of ONE call (never accumulated across calls). */
int sepfwi_pseudo_hessian_arm(const char *para_fname, int gpu_id, int every);
/* result of the most recent armed misfit / gradient call; (nz, nx) float32 each, host or device,
   any of the three may be NULL; SEPFWI_EINVAL "no session" / "no armed call yet" */
int sepfwi_get_pseudo_hessian(const char *para_fname, int gpu_id, float *hLambda, float *hMu, float *hDen);

/*
 * Extension (no counterpart in the reference; no reference run pins it): Born modelling and the Gauss-Newton Hessian-vector product.
 * Given the model m = (Lambda, Mu, Den) and a perturbation v = (dLambda, dMu, dDen) -- all (nz, nx) float32, MPa / kg m^-3, host or
 * device pointers with the conventions of sepfwi_cufd_stream -- the call propagates the scattered field next to the background field
 * (no finite difference, no step size) and returns J v, the first-order change of every gather:
 *   d_ett, d_vx, d_vz   each may be NULL; else the scattered gathers shot after shot in the order of shot_ids, each [nrec_i][nSteps]
 *                       (the layout of Shot_*.bin; column it + 1 holds the state after step it, column 0 is 0).  Every receiver geometry
 *                       and parameter key of the forward pass applies (das_fiber, directional channels, das_gauge_length).  The data-
 *                       conditioning keys (if_win, filter, if_cross_misfit, if_src_update) do NOT alter these raw gathers.
 *   hv_Lambda, hv_Mu, hv_Den   all NULL: J v only.  All set: overwritten with the Gauss-Newton product summed over the call's shots,
 *                       hv = J^T W J v, W = diag(misfit_w_ett, misfit_w_vx, misfit_w_vz) of the parameter file (default (1, 0, 0)) and
 *                       J^T the backward pass of a gradient call.  Sign and weights: hv is the gradient that sepfwi_cufd(calc_id 1) would
 *                       return at m if the observed data were syn(m) - J v; so v^T hv >= 0 up to the inexactness of the reference's adjoint.
 *                       (nz, nx) float32 each, host or device.  One set and the others NULL: SEPFWI_EINVAL.
 *                       Under a parameter file whose live conditioning keys are among if_win and filter the misfit is still quadratic in
 *                       the data, and the same sentence holds for the conditioned misfit: hv = J^T C^T Z C J v, with C = B Wn (per-channel
 *                       windows with weights, or the end taper; then the zero-phase band-pass: sepfwi_condition below) and Z the zeroing of
 *                       time sample 0 that the conditioned residual applies.  d_* stay the raw gathers.
 *                       Under if_envelope_misfit the misfit is a non-linear least-squares problem in the squared envelope, and hv is its
 *                       Gauss-Newton product hv = J^T C^T D^T Z D C J v with D = 2 [diag(s) + diag(H s) H] the derivative of the squared
 *                       envelope at s = C of the BACKGROUND gather (one more sampler launch per time step records it, only under the key):
 *                       symmetric, non-negative, the full Hessian where the residual vanishes; the second-order term of the envelope map is
 *                       left out.  d_* stay the raw gathers, bit for bit those of the file without the key.
 * Refused with SEPFWI_EINVAL before anything is touched: a NULL model, perturbation, stf or para_fname; a bad shot list; the product
 * (hv_* set) under if_cross_misfit (a misfit that is not quadratic in the data), if_src_update (a matching filter that depends on the
 * synthetics) or if_w2_misfit (no least-squares Gauss-Newton form; the message names the key) -- the scattered gathers alone are still served then.  SEPFWI_ECOURANT applies to the
 * background model only.  Under robust_misfit the product is J^T C^T Z W Z C J v, W the IRLS weight at (C obs, C of the background gather):
 * the call records the background gather as under if_envelope_misfit and READS the shot's observed gather from the session's store
 * (sepfwi_set_observed or the files), released with the shot.  Otherwise the session's observed data, its misfit, sepfwi_get_misfit_parts and the pseudo-Hessian state are neither
 * read nor written; sepfwi_get_stats afterwards describes this call (fwd_ms: the Born time loops).
 * Schedule: one shot after the other on the call's stream (hip_stream, NULL: the session's own), synchronous; the batched multi-lane
 * schedule of sepfwi_cufd* is not used.  Option quiet_skip is ignored for this call.  The second field set (18 arrays) is allocated on
 * the first call; a process that never calls this function launches and allocates exactly what it did before.
 */
int sepfwi_born(float *d_ett, float *d_vx, float *d_vz, float *hv_Lambda, float *hv_Mu, float *hv_Den, const float *Lambda, const float *Mu,
                const float *Den, const float *dLambda, const float *dMu, const float *dDen, const float *stf, int gpu_id, int group_size,
                const int *shot_ids, const char *para_fname, void *hip_stream);

/*
 * Extension (no counterpart in the reference; no reference run pins it): the exact discrete adjoint.  J^T as the transpose of the
 * forward operator that sepfwi_born linearises -- coefficients, 1/K and a of the C-PML inside the transposed stencils, residual column
 * nSteps-1 injected, no edge tests in the finalisation (csrc/exact_adjoint.hpp) -- so that <J v, w> = <v, J^T w> to float32 rounding.
 * The reference's backward pass stays the default of every other call, bit for bit.  Results live on
 *   Omega = rows nPml+1 ... nz-nPad-nPml-1, columns nPml+1 ... nx-nPml-1 of the padded (nz, nx) grid
 * (the physical interior without its first row and first column) and are 0 elsewhere.  The mode follows from the inputs:
 *   w_* set (any of w_ett, w_vx, w_vz), dLambda = dMu = dDen = NULL
 *       g = J^T w, no weights and no sign.  w has the layout of sepfwi_born's d_*: [nrec_i][nSteps] shot after shot in the order of
 *       shot_ids; column 0 is ignored.  A component needs a weight in the parameter file (misfit_w_*; ett by default): the session
 *       injects only those.  misfit is untouched.
 *   dLambda, dMu, dDen all set, w_* all NULL
 *       g = P J^T W J P v, P the restriction to Omega (v is read on Omega only), W as sepfwi_born takes it; the background forward pass
 *       is shared between J and J^T.  Symmetric and non-negative.  misfit is untouched.
 *   neither set
 *       g is the exact gradient on Omega of the session's misfit 1/2 sum_c w_c |obs_c - syn_c|^2 (all columns), and *misfit (may be
 *       NULL) is that value, as sepfwi_cufd(calc_id 1) reports it.
 * Every receiver geometry and parameter key of the forward pass applies (das_fiber, directional channels, das_gauge_length, misfit_w_*).
 * Windowed and band-passed data (live conditioning keys among if_win and filter; C and Z as under sepfwi_born):
 *   the product is g = P J^T C^T Z C J P v, still symmetric and non-negative (v^T g = |Z C J P v|^2);
 *   the gradient mode returns the exact gradient on Omega of the conditioned misfit 1/2 |Z (C obs - C syn)|^2 and that value in *misfit,
 *   as a misfit call on the same file reports it;
 *   the w mode is untouched: g = J^T w with w in raw data space -- a caller composes C and C^T through sepfwi_condition.
 * Envelope misfit (if_envelope_misfit; D, H, e as under sepfwi_cufd and sepfwi_born): the product is g = P J^T C^T D^T Z D C J P v
 *   (v^T g = |Z D C J P v|^2); the gradient mode returns the exact gradient on Omega of 1/2 |Z (e(C obs) - e(C syn))|^2 and that value in
 *   *misfit; the w mode is untouched and stays in raw data space (sepfwi_data_misfit / sepfwi_data_gn give the operators to compose).
 * W2 misfit (if_w2_misfit, as under sepfwi_cufd): the gradient mode returns the exact gradient on Omega of 1/2 sum_r w_r W_r and that value
 *   in *misfit; the w mode is untouched; the product (v set) is refused with SEPFWI_EINVAL, as sepfwi_born refuses it.
 * Robust misfit (robust_misfit, as under sepfwi_cufd): the gradient mode returns the exact gradient on Omega of sum phi and that value in
 *   *misfit; the product is g = P J^T C^T Z W Z C J P v with the IRLS weight W (v^T g = |W^1/2 Z C J P v|^2), which reads the observed
 *   store as sepfwi_born does under the key; the w mode is untouched.
 * Refused with SEPFWI_EINVAL before anything is touched: a NULL model, stf, para_fname or output g_*; a partial v; both v and w; a bad
 * shot list; if_cross_misfit or if_src_update in any mode; a w component without a weight.  SEPFWI_ECOURANT applies to the background model.  The
 * gradient of the source time function is returned by sepfwi_adjoint_exact_src (below), not here.  The session's observed data, sepfwi_get_misfit_parts and the pseudo-Hessian state
 * are read but never written; sepfwi_get_stats afterwards describes this call.  Schedule: one shot after the other on the call's
 * stream, synchronous, two launches and one injection per backward time step; the persistent backward loop and the batched schedule
 * are not used (sepfwi_loop_status says so), options img_every and quiet_skip are not consulted.  A process that never calls this
 * function launches and allocates exactly what it did before.
 */
int sepfwi_adjoint_exact(float *misfit, float *g_Lambda, float *g_Mu, float *g_Den, const float *w_ett, const float *w_vx, const float *w_vz,
                         const float *dLambda, const float *dMu, const float *dDen, const float *Lambda, const float *Mu, const float *Den,
                         const float *stf, int gpu_id, int group_size, const int *shot_ids, const char *para_fname, void *hip_stream);

/*
 * Extension (no counterpart in the reference; no reference run pins it): the source time function in Born modelling and in the exact
 * adjoint.  The wavefield is exactly linear in the source, J_s = F (1500^2 dt) T with F the map from injected amplitudes to gathers and T
 * the end taper of the source rows (sepfwi_stf_taper, ratio 0.001: a pointwise window, its own transpose); column nSteps-1 of the
 * source never enters the forward pass.  The yardstick is the forward operator itself: J_s ds is the gathers of stf = ds.
 * sepfwi_born and sepfwi_adjoint_exact are these two functions with the source arguments NULL, launch for launch and bit for bit.
 *   dStf    (group_size, nSteps) float32, host or device; row i belongs to shot_ids[i] -- the local layout of sepfwi_cufd's grad_stf.  A
 *           shot's source couples to that shot only.  The scattered field gets 1500^2 T[it] dStf[it] dt at the source cell where the
 *           background gets its amplitude: the gathers are J [v; ds] = J_m v + J_s ds.  dLambda, dMu, dDen may then be all NULL (v = 0).
 *   g_stf   (group_size, nSteps) float32, host or device, may be NULL; the same layout, so the operator is square.  Overwritten with
 *           the source block of the result:  J_s^T w  /  the fourth block of [P; I] J^T W J [P v; ds]  /  d misfit / d stf =
 *           J_s^T W (syn - obs), by the mode.  Column nSteps-1 is 0.  Formed inside the transposed time loop's own launches: a call
 *           with g_stf issues the launches of the call without it.
 * sepfwi_born_src: the arguments of sepfwi_born, then dStf.  SEPFWI_EINVAL before anything is touched: a partial v; no v and no dStf;
 * dStf together with hv_* (the reference's backward pass is not the transpose of J: use sepfwi_adjoint_exact_src).
 * sepfwi_adjoint_exact_src: the arguments of sepfwi_adjoint_exact, then dStf and g_stf.  v (all three) or dStf or both: the product;
 * w_*: J^T w; none of v, dStf, w: the gradient mode.  SEPFWI_EINVAL before anything is touched: dStf together with w_*; a partial v.
 */
int sepfwi_born_src(float *d_ett, float *d_vx, float *d_vz, float *hv_Lambda, float *hv_Mu, float *hv_Den, const float *Lambda, const float *Mu,
                    const float *Den, const float *dLambda, const float *dMu, const float *dDen, const float *stf, int gpu_id, int group_size,
                    const int *shot_ids, const char *para_fname, void *hip_stream, const float *dStf);
int sepfwi_adjoint_exact_src(float *misfit, float *g_Lambda, float *g_Mu, float *g_Den, const float *w_ett, const float *w_vx, const float *w_vz,
                             const float *dLambda, const float *dMu, const float *dDen, const float *Lambda, const float *Mu, const float *Den,
                             const float *stf, int gpu_id, int group_size, const int *shot_ids, const char *para_fname, void *hip_stream,
                             const float *dStf, float *g_stf);

/* C (transpose = 0) or C^T (transpose != 0) of the parameter file, in place, on gathers laid out like sepfwi_born's d_ett:
   [nrec_i][nSteps] shot after shot in the order of shot_ids; host or device.  C is what the session applies to a synthetic
   axial-strain gather before the residual: per-channel windows with weights (if_win) or the end taper, then the band-pass
   (filter), then the apparent-slowness fan filter across the shot's channels (fk_slowness / fk_mode); the identity when no conditioning
   key is live.  C^T: the fan filter, the band-pass, then the window.  Defined under every key
   (if_cross_misfit and if_src_update select a misfit, not C).  Creates the session as sepfwi_set_observed does; touches no observed
   data, misfit or statistics; synchronous. */
int sepfwi_condition(float *data, int transpose, int gpu_id, int group_size, const int *shot_ids, const char *para_fname, void *hip_stream);

/*
 * The misfit of the parameter file as operators in data space, without any wave propagation: for users of the w mode of
 * sepfwi_adjoint_exact, who compose their own passes.  All gathers are RAW axial-strain gathers laid out like sepfwi_born's d_ett
 * ([nrec_i][nSteps] shot after shot in the order of shot_ids), host or device; inputs are never changed.  Both run the code that a gradient
 * call or a product of the session runs between its two transpositions.  They create the session as sepfwi_condition does, touch no
 * observed data, misfit or statistics, and are synchronous.
 *   sepfwi_data_misfit   *misfit = the file's misfit of (obs, syn), halved as sepfwi_cufd reports it; adj (may be NULL) = the raw-space
 *       adjoint source a = -d misfit / d syn, what the backward pass injects:  C^T Z (C obs - C syn) for the L2 misfit (C = 1 without a
 *       conditioning key),  the adjoint source of the normalised cross-correlation under if_cross_misfit,  C^T D^T Z (e(C obs) - e(C syn))
 *       under if_envelope_misfit,  -1/2 C^T w dW / d(C syn) under if_w2_misfit (W, w as under sepfwi_cufd).  Under if_src_update the matching filter is computed from the call's own (C obs, C syn), shot by shot, as
 *       a gradient call computes it: the misfit is that of the updated synthetics, a is taken with the filter held fixed.  SEPFWI_EINVAL
 *       under weights other than (1, 0, 0).
 *   sepfwi_data_gn       out = the Gauss-Newton operator of the misfit at syn applied to d:  C^T Z C d for the L2 misfit (syn is not
 *       read),  C^T D^T Z D C d under if_envelope_misfit, D at C syn.  Symmetric and non-negative.  SEPFWI_EINVAL under if_cross_misfit,
 *       if_src_update, if_w2_misfit (the transport misfit has no least-squares form in the data), under robust_misfit (the weight needs
 *       the observed data: sepfwi_data_gn_obs) and under weights other than (1, 0, 0).
 *   sepfwi_data_gn_obs   sepfwi_data_gn at (obs, syn).  Under robust_misfit out = C^T Z W Z C d, W = diag(w) the IRLS weight of
 *       (C obs, C syn), 0 on dead traces: symmetric and non-negative; obs is required (SEPFWI_EINVAL if NULL).  Under every other file obs
 *       is not read and may be NULL: the result is that of sepfwi_data_gn bit for bit, and so are the refusals.
 */
int sepfwi_data_misfit(float *misfit, float *adj, const float *obs, const float *syn, int gpu_id, int group_size, const int *shot_ids,
                       const char *para_fname, void *hip_stream);
int sepfwi_data_gn(float *out, const float *syn, const float *d, int gpu_id, int group_size, const int *shot_ids, const char *para_fname,
                   void *hip_stream);
int sepfwi_data_gn_obs(float *out, const float *obs, const float *syn, const float *d, int gpu_id, int group_size, const int *shot_ids,
                       const char *para_fname, void *hip_stream);

/* Drops cached observed data (e.g. after the Shot_*.bin files were rewritten by another tool). */
void sepfwi_invalidate_observed(void);

/*
 * Host helpers exported for parity tests (they are what the session uses internally).
 *   sepfwi_cpml_profiles: the six 1-D C-PML arrays K, a, b, K_half, a_half, b_half of length N.
 *                         Replaces cpmlInit, Src/utilities.cu:243-359.
 *   sepfwi_stf_taper:     in-place sin^2/cos^2 taper of one trace.  Replaces the 5-argument
 *                         cuda_window, Src/utilities.cu:844-884 (ratio 0.001, Src/Src_Rec.cu:137).
 *   sepfwi_shot_split:    start offsets (ngpu+1 ints) of the contiguous shot blocks per GPU.
 *                         Replaces the sepBars logic of Src/Torch_Fwi.cpp:59-60,78-80.
 */
int sepfwi_cpml_profiles(float *K, float *a, float *b, float *K_half, float *a_half,
                         float *b_half, int N, int nPml, float dh, float f0, float dt);
int sepfwi_stf_taper(float *trace, int nt, float dt, float ratio);
int sepfwi_shot_split(int group_size, int ngpu, int *starts);

/*
 * Statistics of the most recent sepfwi_cufd* call on (para_fname, gpu_id): kernel time measured
 * with hipEvents on the session's stream, cell-update counts as defined in SURVEY.md section 8(d).
 */
typedef struct sepfwi_stats {
    double fwd_ms;            /* forward time loops, all shots of the call                    */
    double bwd_ms;            /* backward (reconstruction + adjoint + imaging) time loops     */
    double total_ms;          /* whole call, host wall clock                                  */
    double cell_updates;      /* N_c * (nSteps-1) * shots * (1 or 3)                          */
    long long fwd_steps;      /* forward time steps executed                                  */
    long long bwd_steps;      /* backward time steps executed                                 */
    long long launches;       /* kernel launches issued                                       */
                              /* (under a live data-conditioning key the chain of a shot is counted too: one per kernel and one per
                                 hipFFT exec; conditioning an observed gather when it is installed belongs to no call) */
    long long device_bytes;   /* device memory held by the session: every block, at its allocated size, while it is held */
    int n_c;                  /* computed cells per step (nz-nPad)*(nx)  [PML included]       */
    double probe_kernel_us;   /* option "probe">0: mean duration of the sampled k_bwd_b launches (HIP events) */
    long long probe_calls;    /* number of sampled launches                                     */
    long long obs_device_bytes; /* observed-data store: gathers resident in HBM (part of device_bytes)            */
    long long obs_host_bytes;   /* ... and in the pinned host tier (only with a budget, key / option "obs_cache_mb") */
    long long obs_evictions;    /* gathers moved HBM -> host tier since the store was created                       */
    long long persist_steps;    /* backward time steps of the call that ran inside the persistent loop (option bwd_fuse = 4) */
    long long quiet_active;     /* option quiet_skip: row segments of the call's last shot whose stresses ever held a value ...  */
    long long quiet_total;      /* ... of this many (0: the option was off or the shot's receivers are not a fused line)         */
} sepfwi_stats;
int sepfwi_get_stats(const char *para_fname, int gpu_id, sepfwi_stats *out);

/*
 * Extension (no counterpart in the reference, whose driver has one way of running a backward step, Src/libCUFD.cu:545-631):
 * why the most recent backward passes of (para_fname, gpu_id) did NOT run in the persistent time loop -- "" while they did (or no
 * gradient call has asked yet): the grid is too small for the loop's tiles, the configuration cannot be resident at once, the start
 * rendezvous found the GPU busy, ...  Up to len - 1 characters into `why`, always terminated.  For multi-GPU runs: a rank that fell
 * back to per-step launches is 10 % slower than its peers and must be visible (bench.py prints every rank's string).
 */
int sepfwi_loop_status(const char *para_fname, int gpu_id, char *why, int len);

/*
 * Options (process-wide defaults; every sepfwi_cufd* call takes ONE snapshot of them when it starts).  Names, defaults, meaning:
 *   bwd_fuse 4    backward step: 0 the reference's four kernels + injection, 2 two fused launches, 4 the persistent time loop (else 2)
 *   batch 2       shots of a call: 0 one stream per forward lane, 1 batched launches, 2 chosen by grid size
 *   quiet_skip 0  1: updates of 64-cell row segments whose every input is exactly +0 are left out (bit-identical)
 *   obs_cache_mb 0  HBM budget of the observed-data store in MB (0: unlimited; the parameter-file key of the same name wins)
 *   probe 0       > 0: every probe-th backward launch is timed with HIP events (sepfwi_stats.probe_kernel_us)
 *   img_every 1   k > 1: imaging condition on every k-th backward step with weight k dt -- an opt-in quadrature, gradients within
 *                 1e-4 of every-step imaging; the ONLY option that changes results beyond round-off of the parity tolerances
 * Tuning knobs and timing-only switches exist only in a library built with -DSEPFWI_PROBES (csrc/kernels.hip); here they are unknown
 * names.  Returns SEPFWI_EINVAL for unknown names or values; sepfwi_get_option returns the current default or -1.
 */
int sepfwi_set_option(const char *name, int value);
int sepfwi_get_option(const char *name);

/*
 * Fused parameterisation maps for HIP-resident tensors: what the reference's nn.Modules compute with a
 * dozen elementwise torch kernels per iteration on the CPU -- replicate padding (fwi_utils.py:31-44 with the identity
 * resize), mask blend P_m = Mask P_pad + (1 - Mask) P_ref (FWI_ops.py:120-122), the Lame map -- in ONE launch, and the
 * whole chain rule back to the (nz, nx) parameters (Lame derivatives, mask, transpose of the padding) in ONE.
 *   kind: 0 (Vp, Vs, Den) FWI_ops.py:124-125 | 1 (Lambda, Mu, Den) :204 | 2 (IP, IS, Den) :261-262 |
 *         3 (Vp, Vs, IP) :326-328 | 4 (Vp, Vs, IS) :389-391 | 5 (porosity, clay content, water saturation) Voigt-Reuss-Hill
 *         :451-497 | 6 the same triple, Biot-Gassmann :567-611
 *   A, B, C            (nz, nx) physical grid;  *_ref, Mask, Lambda, Mu, Den, gLambda, gMu, gDen:
 *                      (nz + 2 nPml + nPad, nx + 2 nPml) padded grid; gA, gB, gC: (nz, nx).  All float32 row-major DEVICE
 *                      pointers of one device; launched on hip_stream (NULL: the default stream), not synchronised.
 */
int sepfwi_param_forward(int kind, int nz, int nx, int nPml, int nPad, const float *A, const float *B, const float *C,
                         const float *A_ref, const float *B_ref, const float *C_ref, const float *Mask, float *Lambda,
                         float *Mu, float *Den, void *hip_stream);
int sepfwi_param_backward(int kind, int nz, int nx, int nPml, int nPad, const float *A, const float *B, const float *C,
                          const float *A_ref, const float *B_ref, const float *C_ref, const float *Mask,
                          const float *gLambda, const float *gMu, const float *gDen, float *gA, float *gB, float *gC,
                          void *hip_stream);

/*
 * The tangent of the same chain, and the diagonal of a Hessian pulled back through it.  With E the replicate padding,
 * p_m = Mask E p + (1 - Mask) p_ref and map_kind the per-cell map of sepfwi_param_forward,
 *     P = d(Lambda, Mu, Den) / d(A, B, C) = Dmap_kind(p_m) diag(Mask) E,
 * a linear operator from three (nz, nx) arrays to three padded ones.  sepfwi_param_backward is its exact transpose P^T (the same
 * float32 partials up to rounding; <P v, w> = <v, P^T w>), so a Hessian H_m in (Lambda, Mu, Den) becomes H_p = P^T H_m P in the
 * user's parameters (Gauss-Newton: the second-order term of the map is left out).
 *   sepfwi_param_jvp   (dLambda, dMu, dDen) = P (dA, dB, dC): forward-mode differentiation of the float32 operation list of the
 *                      forward map, one launch over the padded grid.  dA, dB, dC: (nz, nx); each may be NULL, a field that is not
 *                      inverted, read as 0 -- bit for bit the result with an array of zeros.  No special cases: where the
 *                      forward map divides by zero the tangent is IEEE inf / nan.  0 wherever Mask is 0.
 *   sepfwi_param_diag  (hA, hB, hC) = diag(P^T diag(hLambda, hMu, hDen) P):
 *                      hA[s] = sum over the padded cells o that replicate s of Mask(o)^2 sum_k (d m_k / d A at o)^2 h_k(o),
 *                      e.g. the diagonal pseudo-Hessian of sepfwi_get_pseudo_hessian in the user's parameters.  One launch over the
 *                      physical grid and one over its rim (fixed summation order, no atomics), as sepfwi_param_backward.
 * Arrays, sizes, kinds, stream and errors as above (a bad kind or size: SEPFWI_EINVAL before any device is touched).
 */
int sepfwi_param_jvp(int kind, int nz, int nx, int nPml, int nPad, const float *A, const float *B, const float *C,
                     const float *A_ref, const float *B_ref, const float *C_ref, const float *Mask, const float *dA,
                     const float *dB, const float *dC, float *dLambda, float *dMu, float *dDen, void *hip_stream);
int sepfwi_param_diag(int kind, int nz, int nx, int nPml, int nPad, const float *A, const float *B, const float *C,
                      const float *A_ref, const float *B_ref, const float *C_ref, const float *Mask, const float *hLambda,
                      const float *hMu, const float *hDen, float *hA, float *hB, float *hC, void *hip_stream);

/*
 * Model regularisation (an extension without a counterpart in the reference, which has data terms only): damping towards a prior,
 * first-order Tikhonov and Charbonnier-smoothed isotropic total variation of up to three (nz, nx) fields, its gradient and its EXACT
 * Hessian-vector product (symmetric and non-negative: R is convex; not the lagged-diffusivity approximation).  For every field k
 * with p[k] != NULL (a NULL field is skipped), with s = scale[k] and W the cell weights (NULL: 1):
 *     q  = (p - p0) / s
 *     gx(i,j) = (p(i,j+1) - p(i,j)) / (s dx)    0 in the last column         gz(i,j) = (p(i+1,j) - p(i,j)) / (s dz)    0 in the last row
 *     n2 = gx^2 + gz^2,   phi = sqrt(n2 + eps^2)
 *     R  = sum over the cells of  W [ alpha q^2 / 2  +  beta n2 / 2  +  gamma (phi - eps) ]         (a constant field costs exactly 0)
 * and the total is the sum over the fields.  Gradient, in gather form, with c = W (beta + gamma / phi), fx = c gx, fz = c gz:
 *     g(i,j)  = W alpha (p - p0) / s^2 - fx(i,j) / (s dx) - fz(i,j) / (s dz) + fx(i,j-1) / (s dx) + fz(i-1,j) / (s dz)
 * Product, with qx, qz the same differences of v and d = gx qx + gz qz:  tx = W (beta qx + gamma (qx / phi - gx d / phi^3)), tz likewise,
 *     Hv(i,j) = W alpha v / s^2 - tx(i,j) / (s dx) - tz(i,j) / (s dz) + tx(i,j-1) / (s dx) + tz(i-1,j) / (s dz)
 * (a predecessor that does not exist contributes nothing).  One launch over the three fields, one thread per cell, no atomics;
 * float32 with a fixed operation list (csrc/regularizer.hip); the cell energies are summed in double, block partials first and
 * then one block in a fixed order, so the same input gives the same bits.  With gamma[k] == 0 nothing of field k depends on eps.
 *   p, p0, v, g, hv     triples of (nz, nx) float32 row-major arrays, W one such array: host or device memory (of one device), in any
 *                       mix; host arrays are staged and the call then synchronises the stream, device arrays are only enqueued.
 *                       p0[k] may be NULL when alpha[k] == 0.
 *   value               the total R as a double, host or device pointer; value, g or entries of g may be NULL (not computed).
 *   v[k] == NULL        (product) field k is not perturbed: hv[k], when given, is zeros.  There is no coupling between fields.
 * SEPFWI_EINVAL before any device is touched: nz or nx < 1; a negative or non-finite alpha / beta / gamma of a given field;
 * scale, dx or dz <= 0; eps <= 0 while some gamma > 0; alpha[k] > 0 without p0[k]; v[k] for a field without p[k]; all fields NULL.
 */
int sepfwi_regularizer(int nz, int nx, float dx, float dz, const float *const p[3], const float *const p0[3], const float *W,
                       const float alpha[3], const float beta[3], const float gamma[3], const float scale[3], float eps,
                       double *value, float *const g[3], void *hip_stream);
int sepfwi_regularizer_hvp(int nz, int nx, float dx, float dz, const float *const p[3], const float *const p0[3], const float *W,
                           const float alpha[3], const float beta[3], const float gamma[3], const float scale[3], float eps,
                           const float *const v[3], float *const hv[3], void *hip_stream);

/*
 * A model-space smoothing operator S with its exact transpose S^T (an unpinned extension: the reference has nothing of the kind): a
 * separable, normalised Gaussian, truncated at a radius, whose width varies from cell to cell.  All quantities are in cells; fields,
 * widths and normalisers are (nz, nx) float32, x fastest.  sigx, sigz are non-negative widths, rx, rz integer radii in 0 .. 64.
 * Along x, in row i:
 *     Kx[j, m] = 1                                                  for m = j
 *     Kx[j, m] = exp(-(m - j)^2 / (sigx[i,j]^2 + sigx[i,m]^2))      for 0 < |m - j| <= rx with both cells inside the grid, where the sum
 *                                                                   of squares is > 0 (otherwise 0); nothing else is cut off
 *     Kx[j, m] = 0                                                  everywhere else
 *     Nx[i,j]  = sum over m of Kx[j, m]   (>= 1)
 *     Sx u   = (Kx u) / Nx                     Sx^T y = Kx (y / Nx)        Kx is symmetric: the same gather, the scaling moved in front
 * Along z the same down every column with sigz, rz and Nz.  In two dimensions
 *     S = Sx Sz  (the z pass first, then the x pass)             S^T = Sz^T Sx^T  (the order matters: the widths vary)
 * A NULL width array or a radius of 0 makes that axis the identity.  It follows that S 1 = 1 (constants are kept), S = I where both
 * widths are 0, a constant width gives the Gaussian truncated at the radius, <S u, y> = <u, S^T y> exactly, and S S^T is symmetric and
 * non-negative: a legitimate preconditioner for conjugate gradients, and p = p_ref + s S y a change of variables with gradient s S^T g.
 *   sepfwi_smooth_plan    inv_nx = 1 / Nx and inv_nz = 1 / Nz from the widths (one launch); an axis with a NULL width array is left alone.
 *   sepfwi_smooth_apply   out[k] = S in[k] (transpose == 0) or S^T in[k] (transpose != 0) for every field k with in[k] != NULL, with the
 *                         inv_* arrays that sepfwi_smooth_plan made for the same widths and radii.  in[k] == out[k] is allowed.  Every
 *                         pass is a gather, one thread per cell, no atomics: the same input gives the same bits, and three fields in
 *                         one call the bits of three calls.  At most two launches; the intermediate lives in a grow-only block per
 *                         (device, stream) that sepfwi_release_all frees.  float32 with a fixed operation list (csrc/smoother.hip).
 * Arrays are host or device memory (of one device), in any mix; host arrays are staged and the call then synchronises the stream, device
 * arrays are only enqueued on hip_stream.
 * SEPFWI_EINVAL before anything is touched: nz or nx < 1; a radius outside 0 .. 64; a width array without its inv_* array; all three
 * fields NULL (or a NULL triple); in[k] without out[k] or out[k] without in[k]; arrays on different devices.
 */
int sepfwi_smooth_plan(int nz, int nx, int rx, int rz, const float *sigx, const float *sigz, float *inv_nx, float *inv_nz,
                       void *hip_stream);
int sepfwi_smooth_apply(int nz, int nx, int rx, int rz, const float *sigx, const float *sigz, const float *inv_nx, const float *inv_nz,
                        int transpose, const float *const in[3], float *const out[3], void *hip_stream);

/*
 * Test hook: wavefield `which` (0..4: vz, vx, szz, sxx, sxz; 5..9: their adjoint twins; 10..14: the scattered fields of the last
 * sepfwi_born call) of forward lane `lane` as the last sepfwi_cufd* / sepfwi_born call on (para_fname, gpu_id) left it, dense (nz - nPad, nx) row-major float32, host or device pointer.
 * After a gradient call the forward fields are the reverse-time RECONSTRUCTION run back to time step 0, i.e. they must
 * have returned to the zero initial state up to float32 round-off: the size-independent parity
 * property checked at the full 2000 x 1000 x 4000 size, where the CPU oracle cannot go.
 */
int sepfwi_debug_field(const char *para_fname, int gpu_id, int lane, int which, float *out);

/*
 * Test hook: the bytes of device memory and of pinned host memory that the library holds in this process right now, over all its
 * sessions and devices (every allocation of the library goes through one seam that counts them).  After sepfwi_release_all both are
 * back where they were before the first session.
 */
int sepfwi_debug_live_bytes(long long *device, long long *pinned);

#ifdef __cplusplus
}
#endif
#endif /* SEPFWI_H_ */
