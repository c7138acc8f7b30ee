// smoother.hpp -- a model-space smoothing operator S with its exact transpose (smoother.hip): a separable, normalised, truncated
// Gaussian whose width varies from cell to cell, applied to up to three (nz, nx) fields.  The operator is written out in
// include/sepfwi.h (sepfwi_smooth_plan / sepfwi_smooth_apply).
#pragma once
#include <hip/hip_runtime.h>

namespace sepfwi {

constexpr int kSmoothMaxRadius = 64;

// One call's geometry as the C ABI takes it.  An axis whose width array is NULL or whose radius is 0 is the identity.
struct SmoothGeom {
    int nz, nx, rx, rz;
    const float *sigx, *sigz;
};

// inv_nx = 1 / Nx and inv_nz = 1 / Nz of the widths (an axis without a width array is left alone).  Arrays may be host or device
// memory; validates before it touches a device (std::invalid_argument), stages what is not on the device and synchronises the
// stream only when something has to reach host memory.
void run_smooth_plan(const SmoothGeom &g, float *inv_nx, float *inv_nz, hipStream_t st);

// out = S in (transpose false: the z pass, then the x pass) or S^T in (the x pass, then the z pass), field by field; a NULL field is
// skipped, in[k] == out[k] is allowed.  At most two launches; the intermediate of three fields is a workspace of model_call.hpp.
void run_smooth_apply(const SmoothGeom &g, const float *inv_nx, const float *inv_nz, bool transpose, const float *const *in,
                      float *const *out, hipStream_t st);

}  // namespace sepfwi
