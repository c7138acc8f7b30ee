// w2_misfit.hpp -- the trace-wise quadratic Wasserstein (W2) misfit of the conditioning chain (parameter key if_w2_misfit;
// w2_misfit.hip).  Engquist & Froese 2014; Yang et al. 2018: every trace is made a probability density in time, and the misfit is
// the squared transport distance between the synthetic and the observed density.  No counterpart in the reference.
//
// Per trace of n = nt samples, o = C obs and s = C syn (float32), t_i = i dt, i = 1 ... n - 1 (sample 0 carries no mass: the chain's Z;
// it is the node of the CDFs with value 0 at t_0):
//     A        max |o| over the whole trace.  A == 0: a dead trace, W = 0 and res = 0
//     q(x)     softplus(beta x / A) = max(z, 0) + log1p(exp(-|z|)): positive, and scaled by the OBSERVED trace alone -- a constant under
//              differentiation, and a synthetic of the wrong amplitude is still penalised
//     f, g     q(s) / sum q(s), q(o) / sum q(o);  F, G their prefix sums, each divided by its own last entry (the last node is exactly 1)
//     j(i)     the first j >= 1 with G_j >= F_i (a lower bound; G_{n-1} = 1 bounds it)
//     T_i      t_{j-1} + dt (F_i - G_{j-1}) / g_j: the linear interpolation of the inverse of G at F_i
//     W        sum_i f_i (t_i - T_i)^2
//     res      -1/2 w dW/ds:  c_i = 2 f_i (T_i - t_i) dt / g_j(i),  psi_k = (t_k - T_k)^2 + sum_{i >= k} c_i,
//              dW/dq(s)_k = (psi_k - sum_l f_l psi_l) / sum q(s),  dW/ds_k = sigmoid(beta s_k / A) (beta / A) dW/dq(s)_k;  res_0 = 0
// ARITHMETIC: the map is ill-conditioned in its inputs (1 / g and the suffix sums amplify a relative 1e-7 of the traces to 1e-5 of res),
// so every quantity from z = beta x / A onwards is double and res is rounded to float32 ONCE, like k_cross_adjoint's.  No floating-point
// atomics: the same input gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace sepfwi {

constexpr int kW2Planes = 5;  // double scratch planes of [cap][nt] each: F (then (t - T)^2, then psi), G, q(o), q(s), c

// One workgroup of 256 threads per trace of the [nrec][nt] gathers.  weights == nullptr: w_r = 1, else weights[r] * src_weight (a float
// product, as cross_residual's).  scratch: kW2Planes planes of `plane` doubles, plane >= nrec * nt; wsum[r] = w_r W_r.
void launch_w2_trace(hipStream_t st, int nt, int nrec, const float *obs, const float *syn, float *res, const float *weights, float src_weight,
                     float dt, double beta, double *scratch, size_t plane, double *wsum);

}  // namespace sepfwi
