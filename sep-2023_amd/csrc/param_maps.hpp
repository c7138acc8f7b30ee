// param_maps.hpp -- fused parameterisation maps (param_maps.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace sepfwi {

// which triple of user parameters (A, B, C) the module inverts for; numbering is part of the C ABI (include/sepfwi.h)
enum ParamKind {
    PARAM_VP_VS_DEN = 0,   // FWI                FWI_ops.py:66-127
    PARAM_LAM_MU_DEN = 1,  // FWI_Lame_Den       FWI_ops.py:145-204
    PARAM_IP_IS_DEN = 2,   // FWI_IP_IS_Den      FWI_ops.py:208-266
    PARAM_VP_VS_IP = 3,    // FWI_Vp_Vs_IP       FWI_ops.py:270-330
    PARAM_VP_VS_IS = 4,    // FWI_Vp_Vs_IS       FWI_ops.py:333-393
    PARAM_ROCK_VRH = 5,       // FWI_Rock_Physics_VRH       FWI_ops.py:401-497   (A, B, C) = (porosity, clay content, water saturation)
    PARAM_ROCK_GASSMANN = 6,  // FWI_Rock_Physics_gassmann  FWI_ops.py:504-619
    PARAM_KINDS = 7
};

// One call's arguments, by value into the kernels.  (nz, nx) is the physical grid of A, B, C; (nzp, nxp) = (nz + 2 nPml + nPad,
// nx + 2 nPml) the padded one of the reference model, the mask and (Lambda, Mu, Den).
struct ParamArgs {
    int kind, nz, nx, nPml, nzp, nxp;
    const float *A, *B, *C, *A_ref, *B_ref, *C_ref, *Mask;
    const float *in[3];  // what the map is applied to, on the grid it lives on (none for the forward map)
    float *out[3];
};

void launch_param_fwd(hipStream_t st, const ParamArgs &p);  // out = (Lambda, Mu, Den), padded
void launch_param_bwd(hipStream_t st, const ParamArgs &p);  // in = dL/d(Lambda, Mu, Den), padded -> out = dL/d(A, B, C)
// the tangent P = Dmap(p_m) diag(Mask) E of the chain (launch_param_bwd is its transpose); each of in = (dA, dB, dC) may be NULL (= 0)
void launch_param_jvp(hipStream_t st, const ParamArgs &p);
// diag(P^T diag(h) P): in = h on the padded grid -> out on the (nz, nx) grid, rim sum and Mask^2 included
void launch_param_diag(hipStream_t st, const ParamArgs &p);

}  // namespace sepfwi
