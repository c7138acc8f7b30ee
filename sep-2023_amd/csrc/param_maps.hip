// param_maps.hip -- the parameterisation maps of the callers of the operator boundary, fused: user parameters on the
// physical (nz, nx) grid -> replicate padding -> mask blend with the reference model -> (Lambda [MPa], Mu [MPa], Den) on the
// padded grid in ONE launch, and the whole chain rule back (Lame derivatives, mask, transpose of the padding) in one
// launch over the grid plus a small one over its rim.
//
// Replaces, for HIP-resident tensors, the ~20 elementwise torch kernels over 3 x 9 MB that the reference's modules issue per
// iteration on the CPU (DAS_Waveform_Inversion/Ops/FWI/FWI_ops.py:116-127 FWI, :194-204 FWI_Lame_Den, :256-266 FWI_IP_IS_Den,
// :319-330 FWI_Vp_Vs_IP, :381-393 FWI_Vp_Vs_IS; padding fwi_utils.py:31-44 with nz == nz_orig, i.e. the identity resize):
//
//     P_pad  = replicate_pad(P)                                   (fwi_utils.py:40-43)
//     P_m    = Mask * P_pad + (1 - Mask) * P_ref                   (FWI_ops.py:120-122)
//     Lambda, Mu, Den = map_kind(A_m, B_m, C_m)                    (FWI_ops.py:124-125, ...)
//
// Same float32 operation order as the torch expressions (the library is built with -ffp-contract=off), divisions are
// IEEE divisions, so the forward map equals the CPU torch result bit for bit; the backward sums the padding strips in a
// fixed order (torch's replication_pad backward adds in another one: equal to rounding).
//
// The linearised chain (no counterpart in the reference): its tangent P = Dmap_kind(p_m) diag(Mask) E in one launch over the padded
// grid (k_param_jvp; the backward launch above is P^T), and diag(P^T diag(h) P) in the backward's launch structure (k_param_diag,
// k_param_diag_rim: param_cell and param_rim with another per-cell term), both from map_jvp, forward-mode differentiation of the same
// float32 operation lists.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "param_maps.hpp"

namespace sepfwi {

namespace {

struct Triple {
    float a, b, c;
};

// ---- rock-physics maps (phi, cc, sw) -> (Lambda [MPa], Mu [MPa], Den): FWI_ops.py:451-497 (Voigt-Reuss-Hill) and :567-611
// (Biot-Gassmann on a consolidation-parameter frame).  Constants as the reference writes them (double products rounded to
// float32 where torch multiplies a float32 tensor by a Python scalar); every operation is the float32 operation of the torch
// expression, in its order.  The chain rule is reverse-mode differentiation of exactly that operation list (what autograd does),
// including its forms of the quotient rule (-g (a/b)/b), the reciprocal rule (-g r r) and the square-root rule (g / (2 r)).
constexpr float RK_KQ = (float)(37.00 * 1e9), RK_KC = (float)(21.00 * 1e9), RK_KW = (float)(2.25 * 1e9), RK_KH = (float)(0.04 * 1e9);
constexpr float RK_MUQ = (float)(44.00 * 1e9), RK_MUC = (float)(10.00 * 1e9);
constexpr float RK_RHOQ = (float)(2.65 * 1e3), RK_RHOC = (float)(2.55 * 1e3), RK_RHOW = (float)(1.00 * 1e3), RK_RHOH = (float)(0.10 * 1e3);
constexpr float RK_CS = 20.0f, RK_CS15 = (float)(1.5 * 20.0), RK_23 = (float)(2. / 3.);

struct VrhMid {  // intermediates of the VRH map that its chain rule needs
    float omp, omc, oms, ks_v, kf_v, r1, r2, kr, ms, rho_f, rho_s;
};
__device__ __forceinline__ Triple vrh_fwd(float a, float b, float c, VrhMid &q) {
    q.omp = 1.0f - a;
    q.omc = 1.0f - b;
    q.oms = 1.0f - c;
    q.ks_v = RK_KC * b + RK_KQ * q.omc;
    q.kf_v = RK_KW * c + RK_KH * q.oms;
    const float kv = q.omp * q.ks_v + a * q.kf_v;                        // FWI_ops.py:463
    q.r1 = b / RK_KC + q.omc / RK_KQ;
    q.r2 = c / RK_KW + q.oms / RK_KH;
    const float kr1 = q.omp * q.r1 + a * q.r2;                          // :464
    q.kr = 1.0f / kr1;
    const float k = 0.5f * (kv + q.kr);
    q.ms = RK_MUC * b + RK_MUQ * q.omc;
    const float mu0 = 0.5f * (q.omp * q.ms + 0.0f);                     // Reuss shear modulus is zero (:468-472)
    q.rho_f = RK_RHOW * c + RK_RHOH * q.oms;
    q.rho_s = RK_RHOC * b + RK_RHOQ * q.omc;
    Triple o;
    o.c = q.rho_f * a + q.rho_s * q.omp;
    o.a = (k - RK_23 * mu0) / 1e6f;                                     // :484-487
    o.b = mu0 / 1e6f;
    return o;
}
__device__ __forceinline__ Triple vrh_bwd(float a, float b, float c, float gl, float gm, float gd) {
    VrhMid q;
    (void)vrh_fwd(a, b, c, q);
    const float gLam0 = gl / 1e6f;
    const float gMu0 = gm / 1e6f + -(gLam0 * RK_23);
    const float gk = gLam0;
    const float gmuv = 0.5f * gMu0;
    const float gkv = 0.5f * gk, gkr = 0.5f * gk;
    const float gkr1 = -gkr * (q.kr * q.kr);
    float gomp = gkv * q.ks_v, ga = gkv * q.kf_v;
    const float gks_v = gkv * q.omp, gkf_v = gkv * a;
    float gb = gks_v * RK_KC, gomc = gks_v * RK_KQ;
    float gc = gkf_v * RK_KW, goms = gkf_v * RK_KH;
    gomp += gkr1 * q.r1;
    ga += gkr1 * q.r2;
    const float gr1 = gkr1 * q.omp, gr2 = gkr1 * a;
    gb += gr1 / RK_KC;
    gomc += gr1 / RK_KQ;
    gc += gr2 / RK_KW;
    goms += gr2 / RK_KH;
    gomp += gmuv * q.ms;
    const float gms = gmuv * q.omp;
    gb += gms * RK_MUC;
    gomc += gms * RK_MUQ;
    const float grho_f = gd * a, grho_s = gd * q.omp;
    ga += gd * q.rho_f;
    gomp += gd * q.rho_s;
    gc += grho_f * RK_RHOW;
    goms += grho_f * RK_RHOH;
    gb += grho_s * RK_RHOC;
    gomc += grho_s * RK_RHOQ;
    Triple o;
    o.a = ga - gomp;
    o.b = gb - gomc;
    o.c = gc - goms;
    return o;
}

struct GasMid {
    float omp, omc, oms, rho_f, k_f, k_s, mu_s, rho_s, d1, q1, k_d, d2, q2, mu_d, e1, e2, e3, e4, e5, e12, dd, denom, u2, u3, u5, num, k_u,
        rho, nA, A, vp, Bq, vs, vp2, vs2, w;
};
__device__ __forceinline__ Triple gas_fwd(float a, float b, float c, GasMid &q) {
    q.oms = 1.0f - c;
    q.omc = 1.0f - b;
    q.omp = 1.0f - a;
    q.rho_f = RK_RHOW * c + RK_RHOH * q.oms;                            // FWI_ops.py:585-589
    q.k_f = RK_KW * c + RK_KH * q.oms;
    q.k_s = RK_KC * b + RK_KQ * q.omc;
    q.mu_s = RK_MUC * b + RK_MUQ * q.omc;
    q.rho_s = RK_RHOC * b + RK_RHOQ * q.omc;
    q.d1 = 1.0f + RK_CS * a;
    q.q1 = q.omp / q.d1;
    q.k_d = q.k_s * q.q1;                                               // :591
    q.d2 = 1.0f + RK_CS15 * a;
    q.q2 = q.omp / q.d2;
    q.mu_d = q.mu_s * q.q2;                                             // :592
    q.e1 = q.omp / a;
    q.e2 = q.k_f / q.k_s;
    q.e3 = q.k_s - q.k_s * a;
    q.e4 = q.k_d / q.e3;
    q.e5 = 1.0f - q.e4;
    q.e12 = q.e1 * q.e2;
    const float Delta = q.e12 * q.e5;                                   // :594
    q.dd = 1.0f + Delta;
    q.denom = a * q.dd;                                                 // :596
    q.u2 = 1.0f + a;
    q.u3 = q.k_d / q.k_s;
    q.u5 = 1.0f - q.u2 * q.u3;
    q.num = a * q.k_d + q.u5 * q.k_f;
    q.k_u = q.num / q.denom;                                            // :598
    q.rho = q.rho_f * a + q.rho_s * q.omp;                              // :602
    q.nA = q.k_u + 0.75f * q.mu_d;
    q.A = q.nA / q.rho;
    q.vp = sqrtf(q.A);                                                  // :603 (0.75, as the reference has it)
    q.Bq = q.mu_d / q.rho;
    q.vs = sqrtf(q.Bq);
    q.vp2 = q.vp * q.vp;
    q.vs2 = q.vs * q.vs;
    q.w = q.vp2 - q.vs2 * 2.0f;
    Triple o;
    o.a = q.rho * q.w / 1e6f;                                           // :609-611
    o.b = q.rho * q.vs2 / 1e6f;
    o.c = q.rho;
    return o;
}
__device__ __forceinline__ Triple gas_bwd(float a, float b, float c, float gl, float gm, float gd) {
    GasMid q;
    (void)gas_fwd(a, b, c, q);
    const float gL0 = gl / 1e6f, gM0 = gm / 1e6f;
    float grho = gL0 * q.w;
    const float gw = gL0 * q.rho;
    const float gvp2 = gw, gvs2 = -gw * 2.0f;
    grho += gM0 * q.vs2;
    const float gvs2b = gM0 * q.rho;
    grho += gd;
    const float gvp = gvp2 * (2.0f * q.vp);
    const float gvs = gvs2 * (2.0f * q.vs) + gvs2b * (2.0f * q.vs);
    const float gA = gvp / (2.0f * q.vp);
    const float gnA = gA / q.rho;
    grho += -gA * (q.A / q.rho);
    const float gk_u = gnA;
    float gmu_d = gnA * 0.75f;
    const float gBq = gvs / (2.0f * q.vs);
    gmu_d += gBq / q.rho;
    grho += -gBq * (q.Bq / q.rho);
    const float grho_f = grho * a, grho_s = grho * q.omp;
    float ga = grho * q.rho_f, gomp = grho * q.rho_s;
    const float gnum = gk_u / q.denom;
    const float gdenom = -gk_u * (q.k_u / q.denom);
    const float gu5 = gnum * q.k_f;
    float gk_f = gnum * q.u5;
    const float gu4 = -gu5;
    const float gu2 = gu4 * q.u3, gu3 = gu4 * q.u2;
    float gk_d = gu3 / q.k_s;
    float gk_s = -gu3 * (q.u3 / q.k_s);
    ga += gu2;
    ga += gnum * q.k_d;
    gk_d += gnum * a;
    ga += gdenom * q.dd;
    const float gDelta = gdenom * a;
    const float ge12 = gDelta * q.e5, ge5 = gDelta * q.e12;
    const float ge1 = ge12 * q.e2, ge2 = ge12 * q.e1;
    const float ge4 = -ge5;
    gk_d += ge4 / q.e3;
    const float ge3 = -ge4 * (q.e4 / q.e3);
    gk_s += ge3;
    const float gksa = -ge3;
    gk_s += gksa * a;
    ga += gksa * q.k_s;
    gk_f += ge2 / q.k_s;
    gk_s += -ge2 * (q.e2 / q.k_s);
    gomp += ge1 / a;
    ga += -ge1 * (q.e1 / a);
    const float gmu_s = gmu_d * q.q2, gq2 = gmu_d * q.mu_s;
    gomp += gq2 / q.d2;
    ga += (-gq2 * (q.q2 / q.d2)) * RK_CS15;
    gk_s += gk_d * q.q1;
    const float gq1 = gk_d * q.k_s;
    gomp += gq1 / q.d1;
    ga += (-gq1 * (q.q1 / q.d1)) * RK_CS;
    float gb = grho_s * RK_RHOC, gomc = grho_s * RK_RHOQ;
    gb += gmu_s * RK_MUC;
    gomc += gmu_s * RK_MUQ;
    gb += gk_s * RK_KC;
    gomc += gk_s * RK_KQ;
    float gc = gk_f * RK_KW, goms = gk_f * RK_KH;
    gc += grho_f * RK_RHOW;
    goms += grho_f * RK_RHOH;
    Triple o;
    o.a = ga - gomp;
    o.b = gb - gomc;
    o.c = gc - goms;
    return o;
}

// (A_m, B_m, C_m) -> (Lambda, Mu, Den), float32, the reference's expression order
__device__ __forceinline__ Triple map_fwd(int kind, float a, float b, float c) {
    Triple o;
    switch (kind) {
        case PARAM_VP_VS_DEN:  // FWI_ops.py:124-125
            o.a = (a * a - 2.0f * (b * b)) * c / 1e6f;
            o.b = (b * b) * c / 1e6f;
            o.c = c;
            break;
        case PARAM_LAM_MU_DEN:  // FWI_ops.py:204
            o.a = a;
            o.b = b;
            o.c = c;
            break;
        case PARAM_IP_IS_DEN:  // FWI_ops.py:261-262
            o.a = (a * a - 2.0f * (b * b)) / c;
            o.b = (b * b) / c;
            o.c = c;
            break;
        case PARAM_VP_VS_IP:  // FWI_ops.py:326-328   (a = Vp, b = Vs, c = IP)
            o.a = c * a - 2.0f * c / a * (b * b);
            o.b = c / a * (b * b);
            o.c = c / a;
            break;
        case PARAM_VP_VS_IS:  // FWI_ops.py:389-391   (a = Vp, b = Vs, c = IS)
            o.a = c / b * (a * a) - 2.0f * c * b;
            o.b = c * b;
            o.c = c / b;
            break;
        case PARAM_ROCK_VRH: {  // (a, b, c) = (phi, cc, sw)
            VrhMid q;
            o = vrh_fwd(a, b, c, q);
            break;
        }
        default: {  // PARAM_ROCK_GASSMANN
            GasMid q;
            o = gas_fwd(a, b, c, q);
            break;
        }
    }
    return o;
}

// (dL/dLambda, dL/dMu, dL/dDen) at a padded cell -> its contribution to (dL/dA_m, dL/dB_m, dL/dC_m)
__device__ __forceinline__ Triple map_bwd(int kind, float a, float b, float c, float gl, float gm, float gd) {
    Triple o;
    switch (kind) {
        case PARAM_VP_VS_DEN:
            o.a = gl * (2.0f * a * c / 1e6f);
            o.b = gl * (-4.0f * b * c / 1e6f) + gm * (2.0f * b * c / 1e6f);
            o.c = gl * ((a * a - 2.0f * (b * b)) / 1e6f) + gm * ((b * b) / 1e6f) + gd;
            break;
        case PARAM_LAM_MU_DEN:
            o.a = gl;
            o.b = gm;
            o.c = gd;
            break;
        case PARAM_IP_IS_DEN:
            o.a = gl * (2.0f * a / c);
            o.b = gl * (-4.0f * b / c) + gm * (2.0f * b / c);
            o.c = -gl * ((a * a - 2.0f * (b * b)) / (c * c)) - gm * ((b * b) / (c * c)) + gd;
            break;
        case PARAM_VP_VS_IP: {
            const float r = b / a;  // Vs / Vp
            o.a = gl * (c + 2.0f * c * r * r) - gm * (c * r * r) - gd * (c / (a * a));
            o.b = gl * (-4.0f * c * r) + gm * (2.0f * c * r);
            o.c = gl * (a - 2.0f * b * r) + gm * (b * r) + gd / a;
            break;
        }
        case PARAM_VP_VS_IS: {
            const float r = a / b;  // Vp / Vs
            o.a = gl * (2.0f * c * r);
            o.b = gl * (-c * r * r - 2.0f * c) + gm * c - gd * (c / (b * b));
            o.c = gl * (a * r - 2.0f * b) + gm * b + gd / b;
            break;
        }
        case PARAM_ROCK_VRH:
            o = vrh_bwd(a, b, c, gl, gm, gd);
            break;
        default:  // PARAM_ROCK_GASSMANN
            o = gas_bwd(a, b, c, gl, gm, gd);
            break;
    }
    return o;
}

// ---- tangents: forward-mode differentiation of exactly the float32 operation lists above, in their order (what torch.func.jvp
// does with the torch expressions).  Quotient rule (dn - q dd) / d with q the quotient the forward pass formed, reciprocal rule
// -dd (r r), square-root rule dA / (2 r).  No special cases: where the forward map divides by zero the tangent is IEEE inf / nan.
__device__ __forceinline__ Triple vrh_jvp(float a, float b, float c, float da, float db, float dc) {
    VrhMid q;
    (void)vrh_fwd(a, b, c, q);
    const float domp = -da, domc = -db, doms = -dc;
    const float dks_v = RK_KC * db + RK_KQ * domc;
    const float dkf_v = RK_KW * dc + RK_KH * doms;
    const float dkv = (domp * q.ks_v + q.omp * dks_v) + (da * q.kf_v + a * dkf_v);
    const float dr1 = db / RK_KC + domc / RK_KQ;
    const float dr2 = dc / RK_KW + doms / RK_KH;
    const float dkr1 = (domp * q.r1 + q.omp * dr1) + (da * q.r2 + a * dr2);
    const float dkr = -dkr1 * (q.kr * q.kr);
    const float dk = 0.5f * (dkv + dkr);
    const float dms = RK_MUC * db + RK_MUQ * domc;
    const float dmu0 = 0.5f * ((domp * q.ms + q.omp * dms) + 0.0f);
    const float drho_f = RK_RHOW * dc + RK_RHOH * doms;
    const float drho_s = RK_RHOC * db + RK_RHOQ * domc;
    Triple o;
    o.c = (drho_f * a + q.rho_f * da) + (drho_s * q.omp + q.rho_s * domp);
    o.a = (dk - RK_23 * dmu0) / 1e6f;
    o.b = dmu0 / 1e6f;
    return o;
}

__device__ __forceinline__ Triple gas_jvp(float a, float b, float c, float da, float db, float dc) {
    GasMid q;
    (void)gas_fwd(a, b, c, q);
    const float doms = -dc, domc = -db, domp = -da;
    const float drho_f = RK_RHOW * dc + RK_RHOH * doms;
    const float dk_f = RK_KW * dc + RK_KH * doms;
    const float dk_s = RK_KC * db + RK_KQ * domc;
    const float dmu_s = RK_MUC * db + RK_MUQ * domc;
    const float drho_s = RK_RHOC * db + RK_RHOQ * domc;
    const float dd1 = RK_CS * da;
    const float dq1 = (domp - q.q1 * dd1) / q.d1;
    const float dk_d = dk_s * q.q1 + q.k_s * dq1;
    const float dd2 = RK_CS15 * da;
    const float dq2 = (domp - q.q2 * dd2) / q.d2;
    const float dmu_d = dmu_s * q.q2 + q.mu_s * dq2;
    const float de1 = (domp - q.e1 * da) / a;
    const float de2 = (dk_f - q.e2 * dk_s) / q.k_s;
    const float de3 = dk_s - (dk_s * a + q.k_s * da);
    const float de4 = (dk_d - q.e4 * de3) / q.e3;
    const float de5 = -de4;
    const float de12 = de1 * q.e2 + q.e1 * de2;
    const float dDelta = de12 * q.e5 + q.e12 * de5;
    const float ddenom = da * q.dd + a * dDelta;
    const float du3 = (dk_d - q.u3 * dk_s) / q.k_s;
    const float du5 = -(da * q.u3 + q.u2 * du3);
    const float dnum = (da * q.k_d + a * dk_d) + (du5 * q.k_f + q.u5 * dk_f);
    const float dk_u = (dnum - q.k_u * ddenom) / q.denom;
    const float drho = (drho_f * a + q.rho_f * da) + (drho_s * q.omp + q.rho_s * domp);
    const float dnA = dk_u + 0.75f * dmu_d;
    const float dA = (dnA - q.A * drho) / q.rho;
    const float dvp = dA / (2.0f * q.vp);
    const float dBq = (dmu_d - q.Bq * drho) / q.rho;
    const float dvs = dBq / (2.0f * q.vs);
    const float dvp2 = (2.0f * q.vp) * dvp;
    const float dvs2 = (2.0f * q.vs) * dvs;
    const float dw = dvp2 - dvs2 * 2.0f;
    Triple o;
    o.a = (drho * q.w + q.rho * dw) / 1e6f;
    o.b = (drho * q.vs2 + q.rho * dvs2) / 1e6f;
    o.c = drho;
    return o;
}

// (dA_m, dB_m, dC_m) at a padded cell -> (dLambda, dMu, dDen) there: the Jacobian of map_fwd at (a, b, c) applied to the tangent
__device__ __forceinline__ Triple map_jvp(int kind, float a, float b, float c, float da, float db, float dc) {
    Triple o;
    switch (kind) {
        case PARAM_VP_VS_DEN: {
            const float t2 = b * b, dt2 = (2.0f * b) * db;
            const float t4 = a * a - 2.0f * t2, dt4 = (2.0f * a) * da - 2.0f * dt2;
            o.a = (dt4 * c + t4 * dc) / 1e6f;
            o.b = (dt2 * c + t2 * dc) / 1e6f;
            o.c = dc;
            break;
        }
        case PARAM_LAM_MU_DEN:
            o.a = da;
            o.b = db;
            o.c = dc;
            break;
        case PARAM_IP_IS_DEN: {
            const float t2 = b * b, dt2 = (2.0f * b) * db;
            const float t4 = a * a - 2.0f * t2, dt4 = (2.0f * a) * da - 2.0f * dt2;
            o.a = (dt4 - (t4 / c) * dc) / c;
            o.b = (dt2 - (t2 / c) * dc) / c;
            o.c = dc;
            break;
        }
        case PARAM_VP_VS_IP: {
            const float t2 = b * b, dt2 = (2.0f * b) * db;
            const float u3 = 2.0f * c / a, du3 = (2.0f * dc - u3 * da) / a;
            const float r = c / a, dr = (dc - r * da) / a;
            o.a = (dc * a + c * da) - (du3 * t2 + u3 * dt2);
            o.b = dr * t2 + r * dt2;
            o.c = dr;
            break;
        }
        case PARAM_VP_VS_IS: {
            const float t1 = a * a, dt1 = (2.0f * a) * da;
            const float r = c / b, dr = (dc - r * db) / b;
            const float w1 = 2.0f * c;
            o.a = (dr * t1 + r * dt1) - ((2.0f * dc) * b + w1 * db);
            o.b = dc * b + c * db;
            o.c = dr;
            break;
        }
        case PARAM_ROCK_VRH:
            o = vrh_jvp(a, b, c, da, db, dc);
            break;
        default:  // PARAM_ROCK_GASSMANN
            o = gas_jvp(a, b, c, da, db, dc);
            break;
    }
    return o;
}

// One padded cell's term of diag(P^T diag(h) P): Mask^2 times the column sums of squares of the map's Jacobian, weighted by h.
// The nine partials are three map_jvp calls on unit tangents.
__device__ __forceinline__ Triple map_diag(int kind, float m, float a, float b, float c, float hl, float hm, float hd) {
    const Triple ja = map_jvp(kind, a, b, c, 1.0f, 0.0f, 0.0f);
    const Triple jb = map_jvp(kind, a, b, c, 0.0f, 1.0f, 0.0f);
    const Triple jc = map_jvp(kind, a, b, c, 0.0f, 0.0f, 1.0f);
    const float mm = m * m;
    Triple o;
    o.a = mm * ((ja.a * ja.a) * hl + (ja.b * ja.b) * hm + (ja.c * ja.c) * hd);
    o.b = mm * ((jb.a * jb.a) * hl + (jb.b * jb.b) * hm + (jb.c * jb.c) * hd);
    o.c = mm * ((jc.a * jc.a) * hl + (jc.b * jc.b) * hm + (jc.c * jc.c) * hd);
    return o;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// What one padded cell adds to its physical cell in the two launches over the physical grid and its rim: from the cell's mask m, the
// blended parameters (a, b, c) and the three inputs there.
struct BwdTerm {  // P^T: the chain rule of the map, times the mask
    __device__ __forceinline__ Triple operator()(int kind, float m, float a, float b, float c, float gl, float gm, float gd) const {
        const Triple d = map_bwd(kind, a, b, c, gl, gm, gd);
        Triple o;
        o.a = m * d.a;
        o.b = m * d.b;
        o.c = m * d.c;
        return o;
    }
};
struct DiagTerm {  // diag(P^T diag(h) P): map_diag carries Mask^2 itself
    __device__ __forceinline__ Triple operator()(int kind, float m, float a, float b, float c, float hl, float hm, float hd) const {
        return map_diag(kind, m, a, b, c, hl, hm, hd);
    }
};

// one thread per PHYSICAL cell: the padded cell that is the cell itself
template <class Term>
__device__ __forceinline__ void param_cell(const ParamArgs &P) {
    const float *__restrict__ A = P.A, *__restrict__ B = P.B, *__restrict__ C = P.C, *__restrict__ Mask = P.Mask;
    const float *__restrict__ A_ref = P.A_ref, *__restrict__ B_ref = P.B_ref, *__restrict__ C_ref = P.C_ref;
    const float *__restrict__ i0 = P.in[0], *__restrict__ i1 = P.in[1], *__restrict__ i2 = P.in[2];
    float *__restrict__ o0 = P.out[0], *__restrict__ o1 = P.out[1], *__restrict__ o2 = P.out[2];
    const int x = blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= P.nx || z >= P.nz) return;
    const size_t s = (size_t)z * P.nx + x, o = (size_t)(z + P.nPml) * P.nxp + (x + P.nPml);
    const float m = Mask[o], w = 1.0f - m;
    const Triple d = Term()(P.kind, m, m * A[s] + w * A_ref[o], m * B[s] + w * B_ref[o], m * C[s] + w * C_ref[o], i0[o], i1[o], i2[o]);
    o0[s] = d.a;
    o1[s] = d.b;
    o2[s] = d.c;
}

// Transpose of the replicate padding: one WAVE per cell of the physical grid's rim adds the padded cells that replicate
// it (a strip of the padding for an edge cell, a rectangle for the four corners; its own cell is done above).  Lanes
// stride over the cells row-major, then a shuffle tree, lane 0 adds: a fixed summation order, no atomics.
template <class Term>
__device__ __forceinline__ void param_rim(const ParamArgs &P) {
    const float *__restrict__ A = P.A, *__restrict__ B = P.B, *__restrict__ C = P.C, *__restrict__ Mask = P.Mask;
    const float *__restrict__ A_ref = P.A_ref, *__restrict__ B_ref = P.B_ref, *__restrict__ C_ref = P.C_ref;
    const float *__restrict__ i0 = P.in[0], *__restrict__ i1 = P.in[1], *__restrict__ i2 = P.in[2];
    float *__restrict__ o0 = P.out[0], *__restrict__ o1 = P.out[1], *__restrict__ o2 = P.out[2];
    const int nz = P.nz, nx = P.nx, nPml = P.nPml;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // rim cell: top row, bottom row, then the two columns
    int z, x;
    if (r < nx) { z = 0; x = r; }
    else if (r < 2 * nx) { z = nz - 1; x = r - nx; }
    else if (r < 2 * nx + (nz - 2)) { z = r - 2 * nx + 1; x = 0; }
    else if (r < 2 * nx + 2 * (nz - 2)) { z = r - 2 * nx - (nz - 2) + 1; x = nx - 1; }
    else return;
    if (nz == 1 && r >= nx) return;  // a one-row grid has one rim row
    if (nx == 1 && r >= 2 * nx && r >= 2 * nx + (nz - 2)) return;
    const size_t s = (size_t)z * nx + x;
    const int Z0 = (z == 0) ? 0 : z + nPml, Z1 = (z == nz - 1) ? P.nzp - 1 : z + nPml;
    const int X0 = (x == 0) ? 0 : x + nPml, X1 = (x == nx - 1) ? P.nxp - 1 : x + nPml;
    const int w_ = X1 - X0 + 1, cnt = (Z1 - Z0 + 1) * w_;
    const float a0 = A[s], b0 = B[s], c0 = C[s];
    float ta = 0.0f, tb = 0.0f, tc = 0.0f;
    for (int k = lane; k < cnt; k += 64) {
        const int Z = Z0 + k / w_, X = X0 + k % w_;
        if (Z == z + nPml && X == x + nPml) continue;  // the cell itself
        const size_t o = (size_t)Z * P.nxp + X;
        const float m = Mask[o];
        if (m == 0.0f) continue;
        const float w = 1.0f - m;
        const Triple d = Term()(P.kind, m, m * a0 + w * A_ref[o], m * b0 + w * B_ref[o], m * c0 + w * C_ref[o], i0[o], i1[o], i2[o]);
        ta += d.a;
        tb += d.b;
        tc += d.c;
    }
    ta = dev::wave_sum(ta), tb = dev::wave_sum(tb), tc = dev::wave_sum(tc);
    if (lane == 0) {
        o0[s] += ta;
        o1[s] += tb;
        o2[s] += tc;
    }
}

}  // namespace

// one thread per PADDED cell
__global__ void k_param_fwd(ParamArgs P) {
    const float *__restrict__ A = P.A, *__restrict__ B = P.B, *__restrict__ C = P.C, *__restrict__ Mask = P.Mask;
    const float *__restrict__ A_ref = P.A_ref, *__restrict__ B_ref = P.B_ref, *__restrict__ C_ref = P.C_ref;
    float *__restrict__ Lam = P.out[0], *__restrict__ Mu = P.out[1], *__restrict__ Den = P.out[2];
    const int X = blockIdx.x * blockDim.x + threadIdx.x, Z = blockIdx.y * blockDim.y + threadIdx.y;
    if (X >= P.nxp || Z >= P.nzp) return;
    const size_t o = (size_t)Z * P.nxp + X;
    const size_t s = (size_t)clampi(Z - P.nPml, 0, P.nz - 1) * P.nx + clampi(X - P.nPml, 0, P.nx - 1);  // replicate padding
    const float m = Mask[o], w = 1.0f - m;
    const Triple r = map_fwd(P.kind, m * A[s] + w * A_ref[o], m * B[s] + w * B_ref[o], m * C[s] + w * C_ref[o]);
    Lam[o] = r.a;
    Mu[o] = r.b;
    Den[o] = r.c;
}

// The tangent of the whole chain, P = Dmap(p_m) diag(Mask) E: one thread per PADDED cell, index math of k_param_fwd.  A NULL dA / dB /
// dC is a field that is not inverted: read as 0.0f through the same arithmetic, so the result equals that of an array of zeros.
__global__ void k_param_jvp(ParamArgs P) {
    const float *__restrict__ A = P.A, *__restrict__ B = P.B, *__restrict__ C = P.C, *__restrict__ Mask = P.Mask;
    const float *__restrict__ A_ref = P.A_ref, *__restrict__ B_ref = P.B_ref, *__restrict__ C_ref = P.C_ref;
    const float *__restrict__ dA = P.in[0], *__restrict__ dB = P.in[1], *__restrict__ dC = P.in[2];
    float *__restrict__ dLam = P.out[0], *__restrict__ dMu = P.out[1], *__restrict__ dDen = P.out[2];
    const int X = blockIdx.x * blockDim.x + threadIdx.x, Z = blockIdx.y * blockDim.y + threadIdx.y;
    if (X >= P.nxp || Z >= P.nzp) return;
    const size_t o = (size_t)Z * P.nxp + X;
    const size_t s = (size_t)clampi(Z - P.nPml, 0, P.nz - 1) * P.nx + clampi(X - P.nPml, 0, P.nx - 1);  // replicate padding
    const float m = Mask[o], w = 1.0f - m;
    const float da = dA ? dA[s] : 0.0f, db = dB ? dB[s] : 0.0f, dc = dC ? dC[s] : 0.0f;
    const Triple r = map_jvp(P.kind, m * A[s] + w * A_ref[o], m * B[s] + w * B_ref[o], m * C[s] + w * C_ref[o], m * da, m * db, m * dc);
    dLam[o] = r.a;
    dMu[o] = r.b;
    dDen[o] = r.c;
}

// the transpose P^T and diag(P^T diag(h) P) share one launch structure: the physical grid, then its rim
__global__ void k_param_bwd(ParamArgs P) { param_cell<BwdTerm>(P); }
__global__ void k_param_bwd_rim(ParamArgs P) { param_rim<BwdTerm>(P); }
__global__ void k_param_diag(ParamArgs P) { param_cell<DiagTerm>(P); }
__global__ void k_param_diag_rim(ParamArgs P) { param_rim<DiagTerm>(P); }

namespace {

const dim3 kTile(64, 4);
dim3 tiles(int nz, int nx) { return dim3((nx + 63) / 64, (nz + 3) / 4); }
dim3 rim_blocks(const ParamArgs &p) { return dim3((2 * p.nx + 2 * (p.nz > 2 ? p.nz - 2 : 0) + 3) / 4); }  // four waves, a rim cell each

}  // namespace

void launch_param_fwd(hipStream_t st, const ParamArgs &p) { hipLaunchKernelGGL(k_param_fwd, tiles(p.nzp, p.nxp), kTile, 0, st, p); }

void launch_param_jvp(hipStream_t st, const ParamArgs &p) { hipLaunchKernelGGL(k_param_jvp, tiles(p.nzp, p.nxp), kTile, 0, st, p); }

void launch_param_bwd(hipStream_t st, const ParamArgs &p) {
    hipLaunchKernelGGL(k_param_bwd, tiles(p.nz, p.nx), kTile, 0, st, p);
    hipLaunchKernelGGL(k_param_bwd_rim, rim_blocks(p), dim3(256), 0, st, p);
}

void launch_param_diag(hipStream_t st, const ParamArgs &p) {
    hipLaunchKernelGGL(k_param_diag, tiles(p.nz, p.nx), kTile, 0, st, p);
    hipLaunchKernelGGL(k_param_diag_rim, rim_blocks(p), dim3(256), 0, st, p);
}

}  // namespace sepfwi

