// exact_adjoint.hpp -- the exact discrete adjoint: J^T as the transpose of the forward operator that born.hpp linearises (session_exact.cpp,
// sepfwi_adjoint_exact).  An extension that no reference run pins: the reference's backward pass (el_*_adj, kept bit for bit as the
// default everywhere) multiplies by the local coefficient OUTSIDE the transposed stencil, drops residual column nSteps-1 and sprays
// the rho / mu images through an always-true edge test.  Its yardstick is mathematics:
// <J v, w> = <v, J^T w> with J from tests/born_ref.py.
//
// Forward half steps on the update region R = [2, n-3]^2 (kernels_bodies.hpp; D- / D+ the staggered differences, ~ the C-PML form
// D~ = D / K + m', m' = b m + a D inside the strips and D~ = D outside):
//   S:  szz += dt ((lam + 2 mu) D~-z vz + lam D~-x vx)   sxx += dt (lam D~-z vz + (lam + 2 mu) D~-x vx)   sxz += dt amu (D~+z vx + D~+x vz)
//   V:  vz  += dt ba (D~+z szz + D~-x sxz)               vx  += dt bb (D~-z sxz + D~+x sxx)
// and column it + 1 of the gathers samples the velocities after V of step it.  Transposed time loop, it = nSteps-2 ... 0, with
// (D-)^T = -D+ and (D+)^T = -D- wherever the differenced quantity is 0 outside R.  The kernels write the adjoint fields on R only, so the
// adjoint stresses are; the adjoint velocities are not: the injection of a channel on the first row or column of R (a directional one:
// on the last, too) adds to one cell outside R, which the forward pass samples as an exact zero.  V^T therefore takes its taps on R only:
//   before the loop    v_ += R^T w[nSteps-1]                                  (the column the reference never injects)
//   k_exact_a (it)     rho image (reverse-time velocity body, unchanged), then V^T:
//                        fz = dt ba v_z, fx = dt bb v_x  at the TAP;  E(tap) = in strip ? f / K(tap) + a(tap) Q(tap) : f
//                        s_zz -= D-z[E1]    s_xx -= D-x[E4]    s_xz -= D+x[E2] + D+z[E3]
//                      and, at the own cell, the adjoint memories of S from the final adjoint stresses:  P <- b P + e
//   injection          v_ += R^T w[it]  for it >= 1 (column 0 is never injected: the forward pass never writes it)
//   k_exact_b (it)     lambda / mu image (reverse-time stress body, unchanged), then S^T:
//                        e1 = dt ((lam+2mu) s_zz + lam s_xx), e2 = dt (lam s_zz + (lam+2mu) s_xx), e3 = dt amu s_xz  at the TAP;
//                        G(tap) = in strip ? e / K(tap) + a(tap) P(tap) : e
//                        v_z -= D+z[G1] + D-x[G4]    v_x -= D+x[G2] + D-z[G3]
//                      and, at the own cell, the adjoint memories of V from the final adjoint velocities:  Q <- b Q + f
// The injection runs BEFORE k_exact_b so that Q sees the injected value (receivers inside a layer); a first k_exact_b in its
// adjoint-only form does the same for column nSteps-1.  Strip membership, 1/K and a are taken at the tap, with the forward kernels'
// own tests: z strips for both, x strip  x < nPml || x > nx-nPml-1  for S and  x < nPml || x > nx-nPml  for V (one column narrower on
// the right, kernels_bodies.hpp:196).  a multiplies P / Q of the tap only inside its strip, so P and Q are kept on the strips
// themselves (the reference's form needs them widened by the stencil radius, stress_adj_apply).  No cell reads a neighbour's value
// that the same launch writes: k_exact_a reads v_ and Q through stencils and writes s_ and P of its own cell, k_exact_b the reverse.
// Media at the taps come from the stored arrays (lam, mu, ave_mu, byc_a, byc_b: the bits the forward kernels use, whether they stream
// or rebuild them); these shifted loads hit the vector L1 (profiles/r04_xtap_probe.txt).
//
// Finalisation on Omega = rows nPml+1 ... zmax, columns nPml+1 ... xmax of the padded grid (the physical interior without its first
// row and first column): the transposes of k_born_media's maps applied to the five raw accumulators
//   gLambda = 1e6 acc_lam      gMu = 1e6 (acc_mu + sum over the four amu points p touching the cell of (amu_p^2 / 4 mu^2) acc_xz_p), 0 where amu_p = 0
//   gDen    = -(ba^2 / 2) acc_a at (z, x) and (z-1, x)  -  (bb^2 / 2) acc_b at (z, x) and (z, x-1)
// and 0 elsewhere.  Accumulators exist on the interior only; a perturbation on Omega couples only at staggered points inside it, and
// every point a cell of Omega gathers from is an interior one -- no edge test is left.
//
// Source block (sepfwi_adjoint_exact_src): the forward pass adds amp[it] = 1500^2 T[it] stf[it] dt to szz and sxx of the source cell after
// S of step it = 0 ... nSteps-2 (T: the end taper of the source rows, a pointwise window, so its own transpose).  The transpose of that
// add is a gather of the adjoint stresses at the source cell as they stand after V^T (k_exact_a) and before S^T of the same step; S^T
// reads them through its taps and never writes them, so ONE lane of k_exact_b(it) stores  g_amp[it] = s_zz + s_xx  -- no launch of its
// own, a plain vector store.  The adjoint-only k_exact_b that primes column nSteps-1 stores nothing: no amplitude follows the last
// velocity update.  The adjoint fields carry the sign of a gradient call's residual (the adjoint source is -w, the imaging condition
// takes the other minus), hence on the host
//   gStf[it] = -1500^2 dt T[it] g_amp[it]   for it <= nSteps-2,      gStf[nSteps-1] = 0
// one row per shot of the call (a shot's source couples to that shot only), the layout of sepfwi_cufd's grad_stf.
//
// A translation unit of its own (exact_adjoint.hip): the field kernels are untouched, and a process that never calls
// sepfwi_adjoint_exact issues exactly the launches and allocates exactly the memory it did before.  The persistent backward loop and
// the batched schedule are not used by this pass: one shot after the other, two launches and one injection per time step.
#pragma once
#include <hip/hip_runtime.h>

#include "fwi_types.hpp"
#include "kernels.hpp"

namespace sepfwi {

// Arrays as bundles (base + k stride n), as the fused backward kernels take them (kernels_step.hpp BwdArgs): <= 80 SGPRs.
struct ExactArgs {
    float *fields;       // vz, vx, szz, sxx, sxz (reconstructed background)
    float *mem;          // the eight adjoint C-PML memories: P1..P4 in the slots of the stress kernels', Q1..Q4 in the velocity kernels'
    float *adj;          // adjoint vz, vx, szz, sxx, sxz
    const float *media;  // lam, mu, ave_mu, byc_a, byc_b, rho
    float *acc;          // lam, mu, xz, a, b
    const float *cz;     // six z profiles of nzc floats, then six x profiles of nx
    size_t n;
};

void launch_exact_a(hipStream_t st, const Grid &g, const KernelOptions &o, const ExactArgs &b, const float *frame_t);
// adjoint_only: S^T and the Q update alone (no reverse-time body, no imaging; frame_t may be null, g_amp_it is not written)
// g_amp_it non-null: one lane stores the source gather of this step there (the header comment, "Source block")
void launch_exact_b(hipStream_t st, const Grid &g, const KernelOptions &o, const ExactArgs &b, float *frame_t, int z_src, int x_src, float src_amp,
                    bool adjoint_only, float *g_amp_it = nullptr);
// dense (nz, nx) outputs, zero outside Omega
void launch_exact_finalize(hipStream_t st, const Grid &g, Media md, ImgAcc acc, float *gLam, float *gMu, float *gDen);
// P_Omega in place on k dense (nz, nx) arrays at stride `dense`
void launch_exact_mask(hipStream_t st, const Grid &g, float *v, int k, size_t dense);

}  // namespace sepfwi
