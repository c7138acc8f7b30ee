// session_exact.cpp -- Session::adjoint_exact / backward_exact: the exact discrete adjoint (exact_adjoint.hpp, sepfwi_adjoint_exact).
//
// One shot after the other on the call's stream, in lane 0 of the session, as Session::born runs: the batched multi-lane schedule is NOT
// used, and neither is the persistent backward loop -- the pass is two launches and one injection per time step (sepfwi_loop_status
// says so after such a call).  It consumes what a gradient call consumes: the shot's residual buffer, the background's saved boundary
// frames, the five imaging accumulators.  Three sources fill the residual buffer:
//   the residual kernels (k_residual, k_geo_residual)  from the session's observed data: the exact gradient (adjoint_exact, no w)
//   k_adjoint_source (geophone.hip)                    from J v: the product P J^T W J P v (Session::born with exact = true)
//   the same kernel                                    from the caller's w: J^T w (adjoint_exact with w)
// Under a parameter file with if_win / filter (C = band-pass . window, Z the zeroing of sample 0) the first becomes
// residual_conditioned: C^T Z (C obs - C syn), the second adjoint_source_conditioned: the product P J^T C^T Z C J P v; the third is
// untouched -- w stays in raw data space (sepfwi_condition applies C).  if_cross_misfit and if_src_update are refused.
// Per shot: a plain forward pass with boundary-frame save (or the Born pass), the adjoint source, then backward_exact:
//   column nSteps-1 injected, Q primed by k_exact_b in its adjoint-only form, and for it = nSteps-2 ... 0
//   k_exact_a, injection of column it (it >= 1; the plans and k_inject of a gradient call), k_exact_b
// with the imaging condition on every step (option img_every is not consulted).  After the last shot k_exact_finalize writes g on Omega.
// Source block (g_stf set, sepfwi_adjoint_exact_src): one lane of k_exact_b(it) stores the adjoint stresses of the source cell into the
// shot's row of the source-gradient buffer a gradient call uses (prepare_buffers allocates and zeroes it for every call with a backward
// pass: nothing new is allocated, no launch is added per step), and write_stf_exact scales the rows on the host after the last shot.
// The session's observed data, misfit parts and pseudo-Hessian state are read but never written.  Stats (fwd_ms, bwd_ms, launches, steps) and device_bytes describe this call.
#include <algorithm>
#include <cstring>
#include <vector>

#include "device_alloc.hpp"
#include "exact_adjoint.hpp"
#include "geophone.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "session.hpp"

namespace sepfwi {

void Session::backward_exact(Call &c, const ShotCtx &x, bool src_gather) {
    hipStream_t st = c.st;
    // the shot's row of source gathers g_amp (prepare_buffers zeroed it; column nSteps-1 is never written: no amplitude follows the last V)
    float *g_amp = src_gather ? stf_grad_.get() + (size_t)x.is * par_.nSteps : nullptr;
    const BwdLane L{st, mem_, adj_, acc_};
    const int nSteps = par_.nSteps;
    const ExactArgs a{x.fld.vz, mem_.dvz_dz, adj_.vz, md_.lam, acc_.lam, pc_.a_z, cells_};
    HIP_OK(hipEventRecord(ev_[2], st));
    backward_init(L);
    if (x.nrec > 0) {  // the column a gradient call never injects, and the adjoint memories of the velocity update that see it
        inject_column(x, L, x.res + (size_t)(nSteps - 1) * x.nres);
        launch_exact_b(st, g_, c.opt, a, nullptr, 0, 0, 0.0f, true);
        cs_.launches += 2;
    }
    for (int it = nSteps - 2; it >= 0; it--) {
        float *frame_t = x.frame + (size_t)it * 5 * (size_t)g_.frame_len;
        const float amp = c.src_scale * x.stf_s[it] * par_.dt;
        launch_exact_a(st, g_, c.opt, a, frame_t);
        if (it >= 1 && x.nrec > 0) {
            inject_column(x, L, x.res + (size_t)it * x.nres);
            cs_.launches++;
        }
        launch_exact_b(st, g_, c.opt, a, frame_t, x.sh->z_src, x.sh->x_src, amp, false, g_amp ? g_amp + it : nullptr);
        cs_.launches += 2;
    }
    HIP_OK(hipEventRecord(ev_[3], st));
    cs_.bwd_steps += (long long)(nSteps - 1);
    cs_.bwd_ms += bracket_ms(2, st);
}

// the finalisation on Omega; in place or staged as write_outputs does it (grad_out)
void Session::write_outputs_exact(Call &c, float *g_Lambda, float *g_Mu, float *g_Den) {
    const GradOut o = grad_out(g_Lambda, g_Mu, g_Den);
    launch_exact_finalize(c.st, g_, md_, acc_, o.dev[0], o.dev[1], o.dev[2]);
    cs_.launches++;
    copy_staged(o, c.st);
}

// The source block of the result from the rows of source gathers (exact_adjoint.hpp): gStf[i][it] = -1500^2 dt T[it] g_amp[i][it], row i
// the call's shot i, T the end taper of prepare_buffers applied to a trace of ones (a pointwise window is its own transpose).  A few
// thousand floats: formed on the host, as write_outputs hands out grad_stf.
void Session::write_stf_exact(Call &c, float *g_stf) {
    const int nSteps = par_.nSteps;
    std::vector<float> h((size_t)c.group_size * nSteps), T((size_t)nSteps, 1.0f);
    if (h.empty()) return;
    HIP_OK(hipMemcpyAsync(h.data(), stf_grad_.get(), h.size() * sizeof(float), hipMemcpyDeviceToHost, c.st));
    HIP_OK(hipStreamSynchronize(c.st));
    stf_taper(T.data(), nSteps, par_.dt, 0.001f);
    for (int i = 0; i < c.group_size; i++)
        for (int it = 0; it < nSteps; it++) {
            float &q = h[(size_t)i * nSteps + it];
            q = it <= nSteps - 2 ? (float)(-(double)c.src_scale * (double)par_.dt * (double)T[it] * (double)q) : 0.0f;
        }
    HIP_OK(hipMemcpy(g_stf, h.data(), h.size() * sizeof(float), hipMemcpyDefault));
}

void Session::adjoint_exact(float *misfit, float *g_Lambda, float *g_Mu, float *g_Den, const float *w_ett, const float *w_vx, const float *w_vz,
                            const float *Lambda, const float *Mu, const float *Den, const float *stf, int group_size, const int *shot_ids,
                            hipStream_t ext_stream, float *g_stf) {
    std::lock_guard<std::mutex> lock(mu_);
    const float *w[4] = {nullptr, w_vx, w_vz, w_ett};  // by component id
    const bool have_w = w_ett || w_vx || w_vz;
    // refusals first: nothing is touched
    if (!traits(par_.misfit).exact_adjoint || par_.if_src_update)
        throw std::invalid_argument("adjoint_exact: not defined for a conditioned misfit with if_cross_misfit or if_src_update (not quadratic in the "
                                    "data); if_win and filter are served");
    static const char *kName[4] = {"", "vx", "vz", "ett"};
    for (int comp = 1; comp <= 3; comp++)
        if (w[comp] && geo_block_[comp] < 0)
            throw std::invalid_argument(std::string("adjoint_exact: w_") + kName[comp] + " needs a component the session injects (parameter key misfit_w_" +
                                        kName[comp] + " > 0)");
    check_shot_ids(group_size, shot_ids);  // (as Session::born)
    Call c = begin_call(ext_stream, group_size, shot_ids);
    c.opt.quiet_skip = 0;
    c.with_adj = true;
    c.if_res = !have_w;  // (ph_every stays 0: an armed pseudo-Hessian is not accumulated by this call)
    hipStream_t st = c.st;
    last_batched_ = false;
    cs_.exact = true;
    if (c.if_res) obs_begin(c);

    prepare_media(c, Lambda, Mu, Den);  // (the Courant guard)
    prepare_buffers(c, stf);

    const int nSteps = par_.nSteps;
    size_t w_off = 0;
    for (int is = 0; is < group_size; is++) {
        ShotCtx x = make_ctx(c, is, stream_lane(0, st), c.if_res);
        x.scratch = false;
        x.comps = c.if_res ? (x.comps & ~1) : 8;  // the gathers the residual needs; with the caller's w none is read (one is sampled, as in a misfit call)

        HIP_OK(hipEventRecord(ev_[0], st));
        forward_init(x);
        const bool inl = forward_inline(c, x);
        for (int it = 0; it <= nSteps - 2; it++) forward_step(c, x, it, inl);
        if (inl) record_column(x, nSteps - 1);
        const size_t cnt = (size_t)x.nrec * nSteps;
        if (c.if_res) {
            cond_on_ ? residual_conditioned(c, x) : residual(x);  // (if_win / filter: C^T Z (C obs - C syn), the misfit of a misfit call)
        } else if (x.nrec > 0) {
            AdjSource q{{}, {}, (size_t)nSteps, 1, x.res, x.nrec, geo_ncomp_};  // the caller's [nrec][nSteps] gathers as they are
            for_active([&](int comp, int b) {
                if (!w[comp]) return;
                const float *src = w[comp] + w_off;
                if (ptr_device(src) != gpu_id_) {  // staged where the forward pass kept this component's gather
                    HIP_OK(hipMemcpyAsync(syn_of(x, comp), src, cnt * sizeof(float), hipMemcpyDefault, st));
                    src = syn_of(x, comp);
                }
                q.src[b] = src;
                q.scale[b] = 1.0f;
            });
            launch_adjoint_source(st, q, nSteps);
            cs_.launches++;
        }
        w_off += cnt;
        HIP_OK(hipEventRecord(ev_[1], st));
        cs_.fwd_steps += (long long)(nSteps - 1);
        cs_.fwd_ms += bracket_ms(0, st);
        if (c.if_res) obs_->release_all();
        backward_exact(c, x, g_stf != nullptr);
    }
    write_outputs_exact(c, g_Lambda, g_Mu, g_Den);
    if (g_stf) write_stf_exact(c, g_stf);
    if (c.if_res && misfit) read_misfit(c, misfit, false);  // as write_outputs forms it -- without touching what sepfwi_get_misfit_parts reports
    end_call(c, true);
}

}  // namespace sepfwi
