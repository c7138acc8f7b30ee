// pseudo_hessian.hpp -- diagonal pseudo-Hessian (source-side illumination per parameter, Shin et al. 2001) accumulated during the
// forward pass: a preconditioner for the three gradients, NOT a Hessian.  An extension that no reference run pins (the reference has
// nothing of the kind); its reference is the definition below evaluated in float64 over the CPU oracle's forward loop
// (tests/pseudo_hessian_ref.py).
//
// Interior = the cell set of the imaging condition, nPml <= z <= Grid::zmax, nPml <= x <= Grid::xmax.  No interior cell takes a C-PML
// branch of the forward kernels, so the derivatives are the plain stencils dminus / dplus (device_common.hpp), the very values
// stress_body / velocity_body compute there.  On forward step it = 0 ... nSteps-2 of a shot with it % every == 0 (weight `every`):
//   between k_stress<FWD> and k_velocity<FWD> -- vz, vx as they stand at the start of the step, szz, sxx, sxz after this step's update
//   and source add:
//     a = D-z vz, b = D-x vx, s = D+z vx + D+x vz          Fz = D+z szz + D-x sxz, Fx = D-z sxz + D+x sxx      (all at index i)
//     E_lam += every (a + b)^2     E_mu += every (4 a^2 + 4 b^2 + s^2)     E_rho += every ((ba^2/2 Fz)^2 + (bb^2/2 Fx)^2)
//   with ba, bb the buoyancies of index i (rebuilt from the density as buoyancies() does).  Summed over the shots of the call:
//     H_lam = 2 (1e6 dt)^2 E_lam     H_mu = (1e6 dt)^2 E_mu     H_rho = dt^2 E_rho
// -- the constants that turn the imaging accumulators into gradients w.r.t. MPa and kg/m^3 in k_finalize_gradients.  These are the
// squared forward-side factors of the three imaging conditions, every factor taken at its own staggered point i WITHOUT the gathers
// (4-point spray of the shear term, 2-point sprays of the density terms) of k_finalize_gradients: a deliberate simplification.
//
// A translation unit of its own (pseudo_hessian.hip): the field kernels are untouched, a session that is not armed issues exactly the
// launches it issued before.
#pragma once
#include <hip/hip_runtime.h>

#include "fwi_types.hpp"

namespace sepfwi {

// One accumulator set (E_lam, E_mu, E_rho), each laid out like a field (nzc + 4 rows of `pitch` floats).
struct PhAcc {
    float *lam, *mu, *rho;
};
constexpr int kPhMaxSets = 4;  // one set per concurrently running forward lane / sub-batch stream (Session::kMaxLanes)
struct PhSets {
    const float *set[kPhMaxSets];  // each [E_lam | E_mu | E_rho] at stride n
    int nsets;
};

// one shot's step into its lane's set (stream schedule); weight = every
void launch_pseudo_hessian(hipStream_t st, const Grid &g, Fields f, Media md, PhAcc acc, float weight);
// the shots of a sub-batch in table order, ONE read-modify-write of the set (batched schedule)
void launch_pseudo_hessian_batch(hipStream_t st, const Grid &g, const ShotDev *shots, int nb, size_t n, Media md, PhAcc acc, float weight);
// sets summed in index order in double, constants applied; dense (nz, nx) outputs, zero outside the interior
void launch_pseudo_hessian_finalize(hipStream_t st, const Grid &g, PhSets sets, size_t n, double c_lam, double c_mu, double c_rho, float *hLam,
                                    float *hMu, float *hDen);

}  // namespace sepfwi
