// capi.cpp -- the extern "C" surface declared in include/sepfwi.h.  Exceptions never cross it: every
// failure becomes an error code plus a thread-local message (the reference printf()s and exit(1)s,
// Src/utilities.h:28-36, which would take the Python interpreter down).
#include <cstdio>
#include <cstring>
#include <string>

#include "kernels.hpp"
#include "model_call.hpp"
#include "param_maps.hpp"
#include "regularizer.hpp"
#include "session.hpp"
#include "smoother.hpp"

using namespace sepfwi;

static thread_local std::string t_last_error = "";

static int fail(int code, const std::string &msg) {
    t_last_error = msg;
    return code;
}

template <class Fn>
static int guarded(Fn &&fn) {
    try {
        fn();
        return SEPFWI_OK;
    } catch (const CourantError &e) {
        return fail(SEPFWI_ECOURANT, e.what());
    } catch (const IoError &e) {
        return fail(SEPFWI_EIO, e.what());
    } catch (const HipError &e) {
        return fail(SEPFWI_EHIP, e.what());
    } catch (const std::invalid_argument &e) {
        return fail(SEPFWI_EINVAL, e.what());
    } catch (const std::runtime_error &e) {
        const char *w = e.what();
        if (std::strncmp(w, "EIO:", 4) == 0) return fail(SEPFWI_EIO, w + 5);
        if (std::strncmp(w, "JSON", 4) == 0 || std::strstr(w, "JSON")) return fail(SEPFWI_EJSON, w);
        return fail(SEPFWI_EINVAL, w);
    } catch (const std::exception &e) {
        return fail(SEPFWI_EINVAL, e.what());
    } catch (...) {
        return fail(SEPFWI_EINVAL, "unknown failure");
    }
}

// The argument checks the entry points share: a parameter file and a sane shot list (where another refusal comes between the two: called
// without the list, then with it, so that the refusals keep their order).
static void check_args(const char *para_fname, int group_size = 0, const int *shot_ids = nullptr) {
    if (!para_fname) throw std::invalid_argument("para_fname is NULL");
    if (group_size < 0 || (group_size > 0 && !shot_ids)) throw std::invalid_argument("bad shot list");
}

// The session of a status query: the one an earlier call made.
static std::shared_ptr<Session> existing_session(const char *para_fname, int gpu_id) {
    if (std::shared_ptr<Session> s = find_session(para_fname, gpu_id)) return s;
    throw std::invalid_argument("no session for this parameter file / gpu");
}

extern "C" {

const char *sepfwi_last_error(void) { return t_last_error.c_str(); }

int sepfwi_version(void) { return 100; }

int sepfwi_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(SEPFWI_EHIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    return n;
}

int sepfwi_cufd_stream(float *misfit, float *grad_Lambda, float *grad_Mu, float *grad_Den, float *grad_stf,
                       const float *Lambda, const float *Mu, const float *Den, const float *stf, int calc_id,
                       int gpu_id, int group_size, const int *shot_ids, const char *para_fname, void *hip_stream,
                       int async) {
    return guarded([&] {
        if (calc_id < 0 || calc_id > 3) throw std::invalid_argument("Invalid calc_id " + std::to_string(calc_id));  // libCUFD.cu:43-46
        check_args(para_fname);
        if (!Lambda || !Mu || !Den || !stf) throw std::invalid_argument("Lambda, Mu, Den and stf must not be NULL");
        check_args(para_fname, group_size, shot_ids);
        if (calc_id == 1 && (!grad_Lambda || !grad_Mu || !grad_Den)) throw std::invalid_argument("gradient outputs must not be NULL for calc_id 1");
        std::shared_ptr<Session> s = get_session(para_fname, gpu_id);
        s->run(misfit, grad_Lambda, grad_Mu, grad_Den, grad_stf, Lambda, Mu, Den, stf, calc_id, group_size, shot_ids,
              (hipStream_t)hip_stream, async != 0);
    });
}

int sepfwi_cufd(float *misfit, float *grad_Lambda, float *grad_Mu, float *grad_Den, float *grad_stf,
                const float *Lambda, const float *Mu, const float *Den, const float *stf, int calc_id, int gpu_id,
                int group_size, const int *shot_ids, const char *para_fname) {
    return sepfwi_cufd_stream(misfit, grad_Lambda, grad_Mu, grad_Den, grad_stf, Lambda, Mu, Den, stf, calc_id, gpu_id,
                              group_size, shot_ids, para_fname, nullptr, 0);
}

void sepfwi_release_all(void) {
    try { release_all_sessions(); } catch (...) {}
    release_model_workspaces();
}

int sepfwi_set_observed(const char *para_fname, int gpu_id, int shot_id, const float *ett, int nrec, int nSteps) {
    return guarded([&] {
        check_args(para_fname);
        get_session(para_fname, gpu_id)->set_observed(shot_id, ett, nrec, nSteps);
    });
}

int sepfwi_set_observed_component(const char *para_fname, int gpu_id, int shot_id, int comp, const float *data, int nrec, int nSteps) {
    return guarded([&] {
        check_args(para_fname);
        if (comp < 1 || comp > 3) throw std::invalid_argument("set_observed_component: comp must be 1 (vx), 2 (vz) or 3 (ett), got " + std::to_string(comp));
        get_session(para_fname, gpu_id)->set_observed(shot_id, data, nrec, nSteps, comp);
    });
}

int sepfwi_get_misfit_parts(const char *para_fname, int gpu_id, double parts[3]) {
    return guarded([&] {
        if (!para_fname || !parts) throw std::invalid_argument("bad arguments");
        existing_session(para_fname, gpu_id)->misfit_parts(parts);
    });
}

int sepfwi_pseudo_hessian_arm(const char *para_fname, int gpu_id, int every) {
    return guarded([&] {
        if (every < 0) throw std::invalid_argument("pseudo_hessian_arm: every must be >= 0, got " + std::to_string(every));
        check_args(para_fname);
        if (every == 0) {  // disarm: nothing to do without a session
            if (std::shared_ptr<Session> s = find_session(para_fname, gpu_id)) s->pseudo_hessian_arm(0);
            return;
        }
        get_session(para_fname, gpu_id)->pseudo_hessian_arm(every);
    });
}

int sepfwi_get_pseudo_hessian(const char *para_fname, int gpu_id, float *hLambda, float *hMu, float *hDen) {
    return guarded([&] {
        check_args(para_fname);
        existing_session(para_fname, gpu_id)->pseudo_hessian_get(hLambda, hMu, hDen);
    });
}

int sepfwi_born_src(float *d_ett, float *d_vx, float *d_vz, float *hv_Lambda, float *hv_Mu, float *hv_Den, const float *Lambda, const float *Mu,
                    const float *Den, const float *dLambda, const float *dMu, const float *dDen, const float *stf, int gpu_id, int group_size,
                    const int *shot_ids, const char *para_fname, void *hip_stream, const float *dStf) {
    return guarded([&] {
        check_args(para_fname);
        if (!Lambda || !Mu || !Den || !stf) throw std::invalid_argument("Lambda, Mu, Den and stf must not be NULL");
        const int n_v = (dLambda ? 1 : 0) + (dMu ? 1 : 0) + (dDen ? 1 : 0);
        if (!dStf && n_v != 3) throw std::invalid_argument("born: dLambda, dMu and dDen must not be NULL");
        if (dStf && n_v != 0 && n_v != 3) throw std::invalid_argument("born: with dStf, dLambda, dMu, dDen must be all NULL or all set");
        check_args(para_fname, group_size, shot_ids);
        const int n_hv = (hv_Lambda ? 1 : 0) + (hv_Mu ? 1 : 0) + (hv_Den ? 1 : 0);
        if (n_hv != 0 && n_hv != 3) throw std::invalid_argument("born: hv_Lambda, hv_Mu, hv_Den must be all NULL (J v only) or all set");
        if (dStf && n_hv == 3)
            throw std::invalid_argument("born: the product with dStf needs the exact adjoint (sepfwi_adjoint_exact_src): the reference's backward pass is "
                                        "not the transpose of J");
        std::shared_ptr<Session> s = get_session(para_fname, gpu_id);
        s->born(d_ett, d_vx, d_vz, hv_Lambda, hv_Mu, hv_Den, Lambda, Mu, Den, dLambda, dMu, dDen, stf, group_size, shot_ids, (hipStream_t)hip_stream,
                false, dStf, nullptr);
    });
}

int sepfwi_born(float *d_ett, float *d_vx, float *d_vz, float *hv_Lambda, float *hv_Mu, float *hv_Den, const float *Lambda, const float *Mu,
                const float *Den, const float *dLambda, const float *dMu, const float *dDen, const float *stf, int gpu_id, int group_size,
                const int *shot_ids, const char *para_fname, void *hip_stream) {
    return sepfwi_born_src(d_ett, d_vx, d_vz, hv_Lambda, hv_Mu, hv_Den, Lambda, Mu, Den, dLambda, dMu, dDen, stf, gpu_id, group_size, shot_ids, para_fname,
                           hip_stream, nullptr);
}

int sepfwi_adjoint_exact_src(float *misfit, float *g_Lambda, float *g_Mu, float *g_Den, const float *w_ett, const float *w_vx, const float *w_vz,
                             const float *dLambda, const float *dMu, const float *dDen, const float *Lambda, const float *Mu, const float *Den,
                             const float *stf, int gpu_id, int group_size, const int *shot_ids, const char *para_fname, void *hip_stream,
                             const float *dStf, float *g_stf) {
    return guarded([&] {
        check_args(para_fname);
        if (!Lambda || !Mu || !Den || !stf) throw std::invalid_argument("Lambda, Mu, Den and stf must not be NULL");
        if (!g_Lambda || !g_Mu || !g_Den) throw std::invalid_argument("adjoint_exact: g_Lambda, g_Mu and g_Den must not be NULL");
        const int n_v = (dLambda ? 1 : 0) + (dMu ? 1 : 0) + (dDen ? 1 : 0);
        if (n_v != 0 && n_v != 3) throw std::invalid_argument("adjoint_exact: dLambda, dMu, dDen must be all NULL or all set");
        const bool have_w = w_ett || w_vx || w_vz;
        if (n_v == 3 && have_w) throw std::invalid_argument("adjoint_exact: either v (the product) or w (J^T w), not both");
        if (dStf && have_w) throw std::invalid_argument("adjoint_exact: either dStf (the product) or w (J^T w), not both");
        check_args(para_fname, group_size, shot_ids);
        std::shared_ptr<Session> s = get_session(para_fname, gpu_id);
        if (n_v == 3 || dStf)
            s->born(nullptr, nullptr, nullptr, g_Lambda, g_Mu, g_Den, Lambda, Mu, Den, dLambda, dMu, dDen, stf, group_size, shot_ids,
                    (hipStream_t)hip_stream, true, dStf, g_stf);
        else
            s->adjoint_exact(misfit, g_Lambda, g_Mu, g_Den, w_ett, w_vx, w_vz, Lambda, Mu, Den, stf, group_size, shot_ids, (hipStream_t)hip_stream, g_stf);
    });
}

int sepfwi_adjoint_exact(float *misfit, float *g_Lambda, float *g_Mu, float *g_Den, const float *w_ett, const float *w_vx, const float *w_vz,
                         const float *dLambda, const float *dMu, const float *dDen, const float *Lambda, const float *Mu, const float *Den,
                         const float *stf, int gpu_id, int group_size, const int *shot_ids, const char *para_fname, void *hip_stream) {
    return sepfwi_adjoint_exact_src(misfit, g_Lambda, g_Mu, g_Den, w_ett, w_vx, w_vz, dLambda, dMu, dDen, Lambda, Mu, Den, stf, gpu_id, group_size, shot_ids,
                                    para_fname, hip_stream, nullptr, nullptr);
}

int sepfwi_condition(float *data, int transpose, int gpu_id, int group_size, const int *shot_ids, const char *para_fname, void *hip_stream) {
    return guarded([&] {
        check_args(para_fname, group_size, shot_ids);
        if (group_size > 0 && !data) throw std::invalid_argument("condition: data must not be NULL");
        get_session(para_fname, gpu_id)->condition(data, transpose != 0, group_size, shot_ids, (hipStream_t)hip_stream);
    });
}

int sepfwi_data_misfit(float *misfit, float *adj, const float *obs, const float *syn, int gpu_id, int group_size, const int *shot_ids,
                       const char *para_fname, void *hip_stream) {
    return guarded([&] {
        check_args(para_fname, group_size, shot_ids);
        if (!misfit) throw std::invalid_argument("data_misfit: misfit must not be NULL");
        if (group_size > 0 && (!obs || !syn)) throw std::invalid_argument("data_misfit: obs and syn must not be NULL");
        get_session(para_fname, gpu_id)->data_misfit(misfit, adj, obs, syn, group_size, shot_ids, (hipStream_t)hip_stream);
    });
}

int sepfwi_data_gn(float *out, const float *syn, const float *d, int gpu_id, int group_size, const int *shot_ids, const char *para_fname,
                   void *hip_stream) {
    return guarded([&] {
        check_args(para_fname, group_size, shot_ids);
        if (group_size > 0 && (!out || !syn || !d)) throw std::invalid_argument("data_gn: out, syn and d must not be NULL");
        get_session(para_fname, gpu_id)->data_gn(out, nullptr, syn, d, group_size, shot_ids, (hipStream_t)hip_stream, false);
    });
}

int sepfwi_data_gn_obs(float *out, const float *obs, const float *syn, const float *d, int gpu_id, int group_size, const int *shot_ids,
                       const char *para_fname, void *hip_stream) {
    return guarded([&] {
        check_args(para_fname, group_size, shot_ids);
        if (group_size > 0 && (!out || !syn || !d)) throw std::invalid_argument("data_gn_obs: out, syn and d must not be NULL");
        get_session(para_fname, gpu_id)->data_gn(out, obs, syn, d, group_size, shot_ids, (hipStream_t)hip_stream, true);  // (obs: checked under the key)
    });
}

void sepfwi_invalidate_observed(void) {
    try { invalidate_observed_all(); } catch (...) {}
}

int sepfwi_cpml_profiles(float *K, float *a, float *b, float *K_half, float *a_half, float *b_half, int N, int nPml,
                         float dh, float f0, float dt) {
    return guarded([&] {
        if (!K || !a || !b || !K_half || !a_half || !b_half || N <= 0 || nPml <= 0) throw std::invalid_argument("bad arguments");
        cpml_profiles(K, a, b, K_half, a_half, b_half, N, nPml, dh, f0, dt);
    });
}

int sepfwi_stf_taper(float *trace, int nt, float dt, float ratio) {
    return guarded([&] {
        if (!trace || nt <= 0) throw std::invalid_argument("bad arguments");
        if (!stf_taper(trace, nt, dt, ratio)) throw std::invalid_argument("Window error 2: taper longer than half the trace");
    });
}

int sepfwi_shot_split(int group_size, int ngpu, int *starts) {
    return guarded([&] {
        if (!starts || ngpu <= 0 || group_size < 0) throw std::invalid_argument("bad arguments");
        if (ngpu > group_size) throw std::invalid_argument("The number of GPUs should be smaller than the number of shots!");  // Torch_Fwi.cpp:49-52
        shot_split(group_size, ngpu, starts);
    });
}

int sepfwi_get_stats(const char *para_fname, int gpu_id, sepfwi_stats *out) {
    return guarded([&] {
        if (!para_fname || !out) throw std::invalid_argument("bad arguments");
        existing_session(para_fname, gpu_id)->stats(out);
    });
}

int sepfwi_loop_status(const char *para_fname, int gpu_id, char *why, int len) {
    return guarded([&] {
        if (!para_fname || !why || len < 1) throw std::invalid_argument("bad arguments");
        const std::string w = existing_session(para_fname, gpu_id)->loop_status();
        std::snprintf(why, (size_t)len, "%s", w.c_str());
    });
}

int sepfwi_debug_field(const char *para_fname, int gpu_id, int lane, int which, float *out) {
    return guarded([&] {
        if (!para_fname || !out) throw std::invalid_argument("bad arguments");
        existing_session(para_fname, gpu_id)->copy_field(lane, which, out);
    });
}

int sepfwi_debug_live_bytes(long long *device, long long *pinned) {
    return guarded([&] {
        if (!device || !pinned) throw std::invalid_argument("bad arguments");
        *device = live_bytes().device.load();
        *pinned = live_bytes().pinned.load();
    });
}

// The fused parameterisation maps run where the tensors live: every array must be device memory of ONE device (the tangents of
// sepfwi_param_jvp may be NULL; the forward map has no `in`), made current for the launch (model_call.hpp) -- they
// run on the autograd thread, whose current device torch's own guards read back with hipGetDevice.
enum class ParamIn { None, Required, Optional };
static int param_call(int kind, int nz, int nx, int nPml, int nPad, const float *A, const float *B, const float *C, const float *A_ref,
                      const float *B_ref, const float *C_ref, const float *Mask, const float *in0, const float *in1, const float *in2,
                      ParamIn in, float *out0, float *out1, float *out2, void *hip_stream,
                      void (*launch)(hipStream_t, const ParamArgs &)) {
    return guarded([&] {
        if (kind < 0 || kind >= PARAM_KINDS) throw std::invalid_argument("param maps: unknown parameterisation " + std::to_string(kind));
        if (nz < 1 || nx < 1 || nPml < 0 || nPad < 0) throw std::invalid_argument("param maps: bad sizes");
        const ParamArgs p{kind, nz, nx, nPml, nz + 2 * nPml + nPad, nx + 2 * nPml, A, B, C, A_ref, B_ref, C_ref, Mask, {in0, in1, in2}, {out0, out1, out2}};
        ModelCall call("param maps", 0, (hipStream_t)hip_stream, true);
        for (const float *q : {A, B, C, A_ref, B_ref, C_ref, Mask}) call.see(q);
        if (in == ParamIn::Required)
            for (const float *q : p.in) call.see(q);
        for (const float *q : p.out) call.see(q);
        if (in == ParamIn::Optional)
            for (const float *q : p.in)
                if (q) call.see(q);
        call.enter();
        launch((hipStream_t)hip_stream, p);
        if (hipGetLastError() != hipSuccess) throw HipError("param map launch failed");
    });
}

int sepfwi_param_forward(int kind, int nz, int nx, int nPml, int nPad, const float *A, const float *B, const float *C,
                         const float *A_ref, const float *B_ref, const float *C_ref, const float *Mask, float *Lambda, float *Mu,
                         float *Den, void *hip_stream) {
    return param_call(kind, nz, nx, nPml, nPad, A, B, C, A_ref, B_ref, C_ref, Mask, nullptr, nullptr, nullptr, ParamIn::None, Lambda, Mu, Den,
                      hip_stream, launch_param_fwd);
}

int sepfwi_param_backward(int kind, int nz, int nx, int nPml, int nPad, const float *A, const float *B, const float *C,
                          const float *A_ref, const float *B_ref, const float *C_ref, const float *Mask, const float *gLambda,
                          const float *gMu, const float *gDen, float *gA, float *gB, float *gC, void *hip_stream) {
    return param_call(kind, nz, nx, nPml, nPad, A, B, C, A_ref, B_ref, C_ref, Mask, gLambda, gMu, gDen, ParamIn::Required, gA, gB, gC, hip_stream,
                      launch_param_bwd);
}

int sepfwi_param_jvp(int kind, int nz, int nx, int nPml, int nPad, const float *A, const float *B, const float *C, const float *A_ref,
                     const float *B_ref, const float *C_ref, const float *Mask, const float *dA, const float *dB, const float *dC,
                     float *dLambda, float *dMu, float *dDen, void *hip_stream) {
    return param_call(kind, nz, nx, nPml, nPad, A, B, C, A_ref, B_ref, C_ref, Mask, dA, dB, dC, ParamIn::Optional, dLambda, dMu, dDen, hip_stream,
                      launch_param_jvp);
}

int sepfwi_param_diag(int kind, int nz, int nx, int nPml, int nPad, const float *A, const float *B, const float *C, const float *A_ref,
                      const float *B_ref, const float *C_ref, const float *Mask, const float *hLambda, const float *hMu,
                      const float *hDen, float *hA, float *hB, float *hC, void *hip_stream) {
    return param_call(kind, nz, nx, nPml, nPad, A, B, C, A_ref, B_ref, C_ref, Mask, hLambda, hMu, hDen, ParamIn::Required, hA, hB, hC, hip_stream,
                      launch_param_diag);
}

int sepfwi_regularizer(int nz, int nx, float dx, float dz, const float *const p[3], const float *const p0[3], const float *W,
                       const float alpha[3], const float beta[3], const float gamma[3], const float scale[3], float eps, double *value,
                       float *const g[3], void *hip_stream) {
    return guarded([&] {
        const RegModel m{nz, nx, dx, dz, p, p0, W, alpha, beta, gamma, scale, eps};
        run_regularizer(m, nullptr, value, g, (hipStream_t)hip_stream);
    });
}

int sepfwi_regularizer_hvp(int nz, int nx, float dx, float dz, const float *const p[3], const float *const p0[3], const float *W,
                           const float alpha[3], const float beta[3], const float gamma[3], const float scale[3], float eps,
                           const float *const v[3], float *const hv[3], void *hip_stream) {
    return guarded([&] {
        if (!v || !hv) throw std::invalid_argument("regularizer: the product needs v and hv");
        const RegModel m{nz, nx, dx, dz, p, p0, W, alpha, beta, gamma, scale, eps};
        run_regularizer(m, v, nullptr, hv, (hipStream_t)hip_stream);
    });
}

int sepfwi_smooth_plan(int nz, int nx, int rx, int rz, const float *sigx, const float *sigz, float *inv_nx, float *inv_nz,
                       void *hip_stream) {
    return guarded([&] {
        const SmoothGeom g{nz, nx, rx, rz, sigx, sigz};
        run_smooth_plan(g, inv_nx, inv_nz, (hipStream_t)hip_stream);
    });
}

int sepfwi_smooth_apply(int nz, int nx, int rx, int rz, const float *sigx, const float *sigz, const float *inv_nx, const float *inv_nz,
                        int transpose, const float *const in[3], float *const out[3], void *hip_stream) {
    return guarded([&] {
        const SmoothGeom g{nz, nx, rx, rz, sigx, sigz};
        run_smooth_apply(g, inv_nx, inv_nz, transpose != 0, in, out, (hipStream_t)hip_stream);
    });
}

int sepfwi_get_option(const char *name) { return get_kernel_option(name); }

int sepfwi_set_option(const char *name, int value) {
    if (set_kernel_option(name, value) == 0) return SEPFWI_OK;
    return fail(SEPFWI_EINVAL, std::string("unknown option or bad value: '") + (name ? name : "") + "'");
}

}  // extern "C"
