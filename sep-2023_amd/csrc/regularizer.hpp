// regularizer.hpp -- model-space regularisation on the device (regularizer.hip): damping towards a prior, first-order Tikhonov and
// Charbonnier-smoothed isotropic total variation of up to three (nz, nx) fields, with the gradient and the exact Hessian-vector
// product.  The functional is written out in include/sepfwi.h (sepfwi_regularizer).
#pragma once
#include <hip/hip_runtime.h>

namespace sepfwi {

// One call's model arguments as the C ABI takes them.  Field k is skipped when p[k] is NULL.
struct RegModel {
    int nz, nx;
    float dx, dz;
    const float *const *p, *const *p0;  // [3] each
    const float *W;
    const float *alpha, *beta, *gamma, *scale;  // [3] each
    float eps;
};

// Value and gradient (v == NULL; value, g or single entries of g may be NULL), or the product (v and out = hv; value NULL).  Arrays
// may be host or device memory; validates before it touches a device (std::invalid_argument), stages what is not on the device and
// synchronises the stream only when something has to reach host memory.  The block partials are a workspace of model_call.hpp.
void run_regularizer(const RegModel &m, const float *const *v, double *value, float *const *out, hipStream_t st);

}  // namespace sepfwi
