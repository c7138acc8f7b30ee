// session_exact.cpp -- Session::adjoint_exact / backward_exact: the exact discrete adjoint (exact_adjoint.hpp, sepfwi_adjoint_exact).
//
// One shot after the other on the call's stream, in lane 0 of the session, as Session::born runs: the batched multi-lane schedule is NOT
// used, and neither is the persistent backward loop -- the pass is two launches and one injection per time step (sepfwi_loop_status
// says so after such a call).  It consumes what a gradient call consumes: the shot's residual buffer, the background's saved boundary
// frames, the five imaging accumulators.  Three sources fill the residual buffer:
//   the residual kernels (k_residual, k_geo_residual)  from the session's observed data: the exact gradient (adjoint_exact, no w)
//   k_born_residual                                    from J v: the product P J^T W J P v (Session::born with exact = true)
//   k_exact_residual                                   from the caller's w: J^T w (adjoint_exact with w)
// Per shot: a plain forward pass with boundary-frame save (or the Born pass), the adjoint source, then backward_exact:
//   column nSteps-1 injected, Q primed by k_exact_b in its adjoint-only form, and for it = nSteps-2 ... 0
//   k_exact_a, injection of column it (it >= 1; the plans and k_inject of a gradient call), k_exact_b
// with the imaging condition on every step (option img_every is not consulted).  After the last shot k_exact_finalize writes g on Omega.
// The session's observed data, misfit parts and pseudo-Hessian state are read but never written; no gradient of the source time
// function is formed.  Stats (fwd_ms, bwd_ms, launches, steps) and device_bytes describe this call.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "device_alloc.hpp"
#include "exact_adjoint.hpp"
#include "geophone.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "session.hpp"

namespace sepfwi {

static bool lives_on(const void *p, int dev) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();  // plain host memory is reported as an error on some ROCm versions
        return false;
    }
    return (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged) && attr.device == dev;
}

void Session::backward_exact(Call &c, const ShotCtx &x) {
    hipStream_t st = c.st;
    const BwdLane L{st, mem_, adj_, acc_};
    const int nSteps = par_.nSteps;
    const ExactArgs a{x.fld.vz, mem_.dvz_dz, adj_.vz, md_.lam, acc_.lam, pc_.a_z, cells_};
    HIP_OK(hipEventRecord(ev_[2], st));
    backward_init(L);
    if (x.nrec > 0) {  // the column a gradient call never injects, and the adjoint memories of the velocity update that see it
        inject_column(x, L, x.res + (size_t)(nSteps - 1) * x.nres);
        launch_exact_b(st, g_, c.opt, a, nullptr, 0, 0, 0.0f, true);
        launches_ += 2;
    }
    for (int it = nSteps - 2; it >= 0; it--) {
        float *frame_t = x.frame + (size_t)it * 5 * (size_t)g_.frame_len;
        const float amp = c.src_scale * x.stf_s[it] * par_.dt;
        launch_exact_a(st, g_, c.opt, a, frame_t);
        if (it >= 1 && x.nrec > 0) {
            inject_column(x, L, x.res + (size_t)it * x.nres);
            launches_++;
        }
        launch_exact_b(st, g_, c.opt, a, frame_t, x.sh->z_src, x.sh->x_src, amp, false);
        launches_ += 2;
    }
    HIP_OK(hipEventRecord(ev_[3], st));
    bwd_steps_ += (long long)(nSteps - 1);
    HIP_OK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, ev_[2], ev_[3]));
    bwd_ms_ += ms;
}

// written in place when the outputs live on this device, staged otherwise (as write_outputs does)
void Session::write_outputs_exact(Call &c, float *g_Lambda, float *g_Mu, float *g_Den) {
    hipStream_t st = c.st;
    const size_t dense = (size_t)par_.nz * (size_t)par_.nx;
    const bool devL = lives_on(g_Lambda, gpu_id_), devM = lives_on(g_Mu, gpu_id_), devD = lives_on(g_Den, gpu_id_);
    float *oL = devL ? g_Lambda : grad_stage_, *oM = devM ? g_Mu : grad_stage_ + dense, *oD = devD ? g_Den : grad_stage_ + 2 * dense;
    launch_exact_finalize(st, g_, md_, acc_, oL, oM, oD);
    launches_++;
    if (!devL) HIP_OK(hipMemcpyAsync(g_Lambda, oL, dense * sizeof(float), hipMemcpyDefault, st));
    if (!devM) HIP_OK(hipMemcpyAsync(g_Mu, oM, dense * sizeof(float), hipMemcpyDefault, st));
    if (!devD) HIP_OK(hipMemcpyAsync(g_Den, oD, dense * sizeof(float), hipMemcpyDefault, st));
}

void Session::adjoint_exact(float *misfit, float *g_Lambda, float *g_Mu, float *g_Den, const float *w_ett, const float *w_vx, const float *w_vz,
                            const float *Lambda, const float *Mu, const float *Den, const float *stf, int group_size, const int *shot_ids,
                            hipStream_t ext_stream) {
    std::lock_guard<std::mutex> lock(mu_);
    const auto t_begin = std::chrono::steady_clock::now();
    const float *w[4] = {nullptr, w_vx, w_vz, w_ett};  // by component id
    const bool have_w = w_ett || w_vx || w_vz;
    // refusals first: nothing is touched
    if (cond_on_)
        throw std::invalid_argument("adjoint_exact: not defined for a conditioned misfit (if_win / filter / if_cross_misfit / if_src_update)");
    static const char *kName[4] = {"", "vx", "vz", "ett"};
    for (int comp = 1; comp <= 3; comp++)
        if (w[comp] && geo_block_[comp] < 0)
            throw std::invalid_argument(std::string("adjoint_exact: w_") + kName[comp] + " needs a component the session injects (parameter key misfit_w_" +
                                        kName[comp] + " > 0)");
    for (int i = 0; i < group_size; i++) {
        const int id = shot_ids[i];
        if (id < 0 || id >= (int)survey_.shots.size() || !survey_.shots[id].present)
            throw std::invalid_argument("shot id " + std::to_string(id) + " is not in the survey file");
    }
    HIP_OK(hipSetDevice(gpu_id_));
    Call c;
    c.opt = kernel_options();
    c.opt.quiet_skip = 0;
    c.st = ext_stream ? ext_stream : own_stream_;
    if (!ext_stream) order_after_null_stream(c.st);
    c.with_adj = true;
    c.if_res = !have_w;  // (ph_every stays 0: an armed pseudo-Hessian is not accumulated by this call)
    c.group_size = group_size;
    c.shot_ids = shot_ids;
    hipStream_t st = c.st;
    launches_ = 0;
    fwd_ms_ = bwd_ms_ = 0.0;
    probe_us_ = 0.0;
    probe_calls_ = 0;
    fwd_steps_ = bwd_steps_ = persist_steps_ = 0;
    quiet_active_ = quiet_total_ = 0;
    quiet_last_ = nullptr;
    last_batched_ = false;
    last_exact_ = true;
    if (c.if_res) {
        const long long mb = par_.obs_cache_mb > 0 ? par_.obs_cache_mb : c.opt.obs_cache_mb;
        obs_->set_budget_bytes(mb * 1000000LL);
        obs_->release_all();
    }

    prepare_media(c, Lambda, Mu, Den);  // (the Courant guard)
    prepare_buffers(c, stf);

    const int nSteps = par_.nSteps;
    size_t w_off = 0;
    for (int is = 0; is < group_size; is++) {
        ShotCtx x = make_ctx(c, is, 0, st, c.if_res);
        x.scratch = false;
        x.comps = c.if_res ? (x.comps & ~1) : 8;  // the gathers the residual needs; with the caller's w none is read (one is sampled, as in a misfit call)

        HIP_OK(hipEventRecord(ev_[0], st));
        forward_init(x);
        const bool inl = forward_inline(c, x);
        for (int it = 0; it <= nSteps - 2; it++) forward_step(c, x, it, inl);
        if (inl) record_column(x, nSteps - 1);
        const size_t cnt = (size_t)x.nrec * nSteps;
        if (c.if_res) {
            residual(x);
        } else if (x.nrec > 0) {
            ExactRes q{};
            q.res = x.res;
            q.nrec = x.nrec;
            q.nblk = joint_ ? geo_ncomp_ : 1;
            for (int comp = 1; comp <= 3; comp++) {
                const int b = geo_block_[comp];
                if (b < 0 || !w[comp]) continue;
                const float *src = w[comp] + w_off;
                if (!lives_on(src, gpu_id_)) {  // staged where the forward pass kept this component's gather
                    HIP_OK(hipMemcpyAsync(syn_of(x, comp), src, cnt * sizeof(float), hipMemcpyDefault, st));
                    src = syn_of(x, comp);
                }
                q.w[b] = src;
            }
            launch_exact_residual(st, q, nSteps);
            launches_++;
        }
        w_off += cnt;
        HIP_OK(hipEventRecord(ev_[1], st));
        fwd_steps_ += (long long)(nSteps - 1);
        HIP_OK(hipStreamSynchronize(st));
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
        fwd_ms_ += ms;
        if (c.if_res) obs_->release_all();
        backward_exact(c, x);
    }
    write_outputs_exact(c, g_Lambda, g_Mu, g_Den);
    if (c.if_res && misfit) {  // as write_outputs forms it -- without touching what sepfwi_get_misfit_parts reports
        double sumsq = 0.0;
        HIP_OK(hipMemcpyAsync(&sumsq, scal_, sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        if (joint_) {
            double s[3] = {0.0, 0.0, 0.0};
            HIP_OK(hipMemcpyAsync(s, geo_sums_, sizeof(s), hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            sumsq = 0.0;
            for (int comp = 1; comp <= 3; comp++) sumsq += (double)par_.weight(comp) * s[comp - 1];
        }
        const float mf = (float)(0.5 * sumsq);
        HIP_OK(hipMemcpy(misfit, &mf, sizeof(float), hipMemcpyDefault));
    }
    HIP_OK(hipStreamSynchronize(st));
    total_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    last_shots_ = group_size;
}

}  // namespace sepfwi
