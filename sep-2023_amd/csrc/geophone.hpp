// geophone.hpp -- particle-velocity (geophone) residuals in misfit and adjoint source, alone or jointly with the axial strain
// (parameter keys "misfit_w_ett" / "misfit_w_vx" / "misfit_w_vz"):
//   misfit = 0.5 sum_shots ( w_ett sum r_ett^2 + w_vx sum r_vx^2 + w_vz sum r_vz^2 ),   r_c = obs_c - syn_c, time sample 0 forced to 0
// vx and vz are sampled at the channel's own cell (k_record / record_gauge_one).  The adjoint source of component c is w_c r_c, added
// to vx_adj / vz_adj of that cell where res_injection_exx adds the strain residual (Src/libCUFD.cu:600-607; the reference ships
// res_injection_vx / _vz, Src/utilities.cu:656-689, and never launches them).
//
// A geophone is a channel with ONE tap (vx | vz, its cell, 1).  The active components of a shot form one concatenated channel list
// -- the ett channels (make_gauge_taps: one-cell, vertical, directional, gauge), then the vx geophones, then the vz geophones -- whose
// channel index is the column of the shot's adjoint-source array [it][C nrec] (C active components, component-major inside a time
// step, already multiplied by w_c).  Its transpose is an InjectPlan (make_gauge_plan): every schedule adds one value per distinct
// target cell and step, the entries summed in that fixed order.
//
// Host part: pure host code (no HIP), unit-tested on the CPU under the sanitizers (tests/native/geophone_check.cpp).  The device side
// (k_geo_residual and its batched twin) lives in geophone.hip; the session takes it only when the weights are not (1, 0, 0).
#pragma once
#include "das_gauge.hpp"

namespace sepfwi {

// Components in the reference's order (libCUFD.cu:216-223): 1 vx, 2 vz, 3 ett.  Column blocks of the adjoint-source array come in
// the order ett, vx, vz.
constexpr int kGeoOrder[3] = {3, 1, 2};

// Number of components with w > 0 and, for comp in 1..3, the column block it owns in the adjoint-source array (-1: inactive).
int geo_blocks(const Params &par, int block_of_comp[4]);

// The concatenated channel list of one shot as taps.  with_*: the components with w > 0; the other arguments as make_gauge_taps.
GaugeTaps make_geophone_taps(int nrec, const int *z_rec, const int *x_rec, const float *sens, bool vertical, float dx_dz, int G, bool with_ett,
                             bool with_vx, bool with_vz);

// One shot of a residual launch: observed and synthetic gathers of the column blocks (time-major [it][nrec]; null: block unused),
// their weights and slots in the sums (comp - 1), the adjoint-source array.
struct GeoResShot {
    const float *obs[3], *syn[3];
    float w[3];
    int slot[3];
    float *res;
    int nrec, nblk;
};

// The same array from something that is not observed data (k_adjoint_source): res[it][b nrec + r] = -(scale_b src_b[r sr + it st]), time
// sample 0 forced to 0, a null src_b: zeros.  The sign is the residual kernels' (obs - syn).  Two callers:
//   the Gauss-Newton product   src_b = J v's gather of the block, time-major (sr 1, st nrec), scale_b = w_b: what the residual kernels leave
//                              for observed data syn - J v
//   J^T w                      src_b = the caller's w_b as sepfwi_born's gathers, [nrec][nSteps] (sr nSteps, st 1), scale_b = 1
struct AdjSource {
    const float *src[3];
    float scale[3];
    size_t sr, st;
    float *res;
    int nrec, nblk;
};

}  // namespace sepfwi
