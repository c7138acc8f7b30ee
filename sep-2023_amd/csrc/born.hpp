// born.hpp -- Born modelling: the linearised forward operator J applied to a model perturbation v = (dLambda, dMu, dDen), propagated
// next to the background field in ONE pair of kernels per time step (session_born.cpp, sepfwi_born).  An extension that no reference
// run pins (the reference has nothing of the kind); its reference is the CPU oracle's own stencil kernels applied to the scattered
// field (tests/born_ref.py), confirmed against central finite differences of the oracle's gathers.
//
// Per-cell perturbed media (k_born_media, five arrays laid out like a field), from v and the session's media of the background:
//   dlam = 1e6 dLambda        dmu = 1e6 dMu
//   damu = (amu^2 / 4) sum_k dmu_k / mu_k^2   over the four cells of the harmonic mean ave_mu (0 where ave_mu is 0: water)
//   dba  = -(ba^2 / 2) (dDen(z+1,x) + dDen(z,x))      dbb = -(bb^2 / 2) (dDen(z,x+1) + dDen(z,x))
// all 0 outside [2, n-3]^2, where the averages are constants.
//
// Scattered field d(vz, vx, szz, sxx, sxz) with eight C-PML memories of its own: same stencils, same recursion (a, b, 1/K do not
// depend on the model), no source term unless the call perturbs the source time function (below), and the cross terms with the
// background's C-PML-modified derivatives D~ of the same step:
//   dszz += dt [(lam + 2 mu) D~z dvz + lam D~x dvx] + dt [(dlam + 2 dmu) D~z vz + dlam D~x vx]            (dsxx likewise)
//   dsxz += dt [amu (D~z dvx + D~x dvz)]            + dt [damu (D~z vx + D~x vz)]
//   dvz  += dt [ba (D~z dszz + D~x dsxz)]           + dt [dba (D~z szz + D~x sxz)]                        (dvx likewise with bb / dbb)
// Source block (sepfwi_born_src, dStf): the wavefield is linear in the source time function, so a perturbation ds of it is a source of
// the scattered field -- dszz and dsxx of the source cell get 1500^2 T[it] ds[it] dt (T: the end taper of the source rows) after the
// update of step it, where the background gets its amplitude.  J [v; ds] = J_m v + J_s ds in one pass; J_s ds alone is the forward
// operator with stf = ds (tests/stf_ref.py).  Without ds the kernel instance is the one that adds nothing.
// The background is advanced by the forward bodies themselves (stress_body / velocity_body, kernels_bodies.hpp): bit for bit a plain
// forward pass, boundary-frame save included.
//
// Bytes per cell and step by arrays streamed (interior): stress 5 fields read + 3 written twice over (64) + lam, mu, dlam, dmu, damu (20)
// = 84 against 2 x 40 of two forward stress updates; velocity 5 + 2 twice over (56) + rho, dba, dbb (12) = 68 against 2 x 32.
//
// A translation unit of its own (born.hip) that shares the device helpers and the launch tiling of the field kernels
// (kernels_device.hpp, tiled()): the field kernels are untouched, and a process that never calls sepfwi_born issues
// exactly the launches and allocates exactly the memory it did before.
#pragma once
#include <hip/hip_runtime.h>

#include "fwi_types.hpp"
#include "kernels.hpp"

namespace sepfwi {

// Arrays as bundles (base + k stride n), as the fused backward kernels take them (kernels_step.hpp BwdArgs).
struct BornArgs {
    float *state;         // background: vz, vx, szz, sxx, sxz, then its 8 C-PML memories
    float *dstate;        // scattered field, same layout
    const float *media;   // lam, mu, ave_mu, byc_a, byc_b, rho
    const float *dmedia;  // dlam, dmu, damu, dba, dbb
    const float *cz;      // six z profiles of nzc floats, then six x profiles of nx
    size_t n;
};

// dense (nz, nx) v + the session's media -> the five perturbed-media arrays
void launch_born_media(hipStream_t st, const Grid &g, const float *Mu_in, const float *dLam_in, const float *dMu_in, const float *dDen_in, Media md,
                       float *dmedia, size_t n);
// one time step: stresses (frame_t non-null: the background's boundary frame of this step is saved first; dsrc_amp non-null: the
// scattered field's own source amplitude of this step, the instance without one writes the bits it always wrote), then velocities
void launch_born_stress(hipStream_t st, const Grid &g, const KernelOptions &o, const BornArgs &b, float *frame_t, int z_src, int x_src, float src_amp,
                        const float *dsrc_amp = nullptr);
void launch_born_velocity(hipStream_t st, const Grid &g, const KernelOptions &o, const BornArgs &b);

}  // namespace sepfwi
