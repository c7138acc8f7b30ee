// robust_misfit.hpp -- the robust data misfits (Huber, Cauchy) of the conditioning chain with a per-trace quantile scale (parameter keys
// robust_misfit / robust_delta / robust_quantile; robust_misfit.hip).  Guitton & Symes 2003; Aravkin et al. 2011: a few samples or
// traces that are off by orders of magnitude (fading channels, interrogator spikes, dropouts) enter linearly or logarithmically, not
// squared.  No counterpart in the reference.
//
// Per trace of nt samples, o = C obs and s = C syn (float32); the live samples are i = 1 ... nt - 1 (sample 0 is zeroed: the chain's Z):
//     A        the order statistic of index k = floor(q (n - 1)), counted from the smallest, of the n = nt - 1 values |o_i|, q =
//              robust_quantile; no interpolation: A is np.sort(np.abs(o[1:]))[k] bit for bit.  From the OBSERVED trace alone: a constant
//              under differentiation, so the misfit is a fixed function of the synthetics.  A == 0: a dead trace, misfit 0, res 0,
//              weight 0 (W2's rule)
//     delta    robust_delta A;   r_i = o_i - s_i;   u = r / delta
//     Huber    phi = delta^2 (u^2 / 2) for |u| <= 1, else delta^2 (|u| - 1/2);   psi = r w,  w = min(1, 1 / |u|)
//     Cauchy   phi = delta^2 / 2 log1p(u^2) (Student-t with the scale absorbed);  psi = r w,  w = 1 / (1 + u^2)
//     misfit   sum_traces sum_i phi;  *acc += 2 sum phi (the driver halves the total, as everywhere)
//     res      psi, res_0 = 0: the sign of l2_residual's output, -d misfit / d s
//     GN       the data-space operator is C^T Z diag(w) Z C with the weight w above taken at the background, in (0, 1] and 0 on dead
//              traces.  This is the IRLS (iteratively reweighted least squares) form, NOT the true Hessian: Huber's true Hessian is 0 on
//              outliers and Cauchy's is indefinite (phi'' < 0 for |u| > 1); the IRLS operator is symmetric and non-negative for both, equals
//              the L2 operator wherever |r| <= delta (Huber) and tends to it as delta -> infinity.
// phi, psi and w are continuous at |u| = 1: a last-bit difference in r cannot flip a result.
// ARITHMETIC: r and everything after it is double, from the float32 inputs; res and the product w d are rounded to float32 ONCE, like
// k_cross_adjoint's and W2's (the weight is never stored: the product kernel forms it in double and rounds w d).  On Huber's plateau psi is
// copysign(delta, r) -- r min(1, 1 / |u|) without its two roundings.  Per-trace sums are double in a fixed order; the selection counts with
// integer LDS atomics, whose result does not depend on their order.  No floating-point atomics: the same input gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace sepfwi {

enum RobustKind { kRobustNone = 0, kRobustHuber = 1, kRobustCauchy = 2 };

// k of the definition for a trace of nt samples, clamped to [0, n - 1] (0 where the trace has no live sample)
int robust_rank(int nt, double quantile);

// One workgroup of 256 threads per trace of the [nrec][nt] gathers: the exact radix select of A (scale[r] = A), then
//   d == nullptr   res = psi and sum[r] = 2 sum_i phi
//   d != nullptr   res = sign Z w Z d, w from (obs, syn) -- the linearised twin; sum is not written
// obs, syn, (d) and res are different gathers.
void launch_robust_trace(hipStream_t st, int nt, int nrec, const float *obs, const float *syn, const float *d, float *res, int kind, double delta,
                         int rank, float sign, float *scale, double *sum);

}  // namespace sepfwi
