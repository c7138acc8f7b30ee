// session_born.cpp -- Session::born: Born modelling J v and the Gauss-Newton product J^T W J v (born.hpp, sepfwi_born).
//
// One shot after the other on the call's stream, in lane 0 of the session (its own state, frames, gathers and residual buffer): the
// batched multi-lane schedule of Session::run is NOT used here -- a Born pass streams twice the arrays of a forward pass, so fewer
// shots share the cache; measuring a batched form is left for later.  Per shot:
//   forward time loop   k_born_stress / k_born_velocity advance background and scattered field; the existing samplers (k_record,
//                       k_record_gauge: one-cell, vertical, directional and gauge channels, vx, vz) read the SCATTERED fields
//   gathers             transposed to [nrec][nSteps] and copied out
//   product only        the residual buffer is filled with -(w_c dsyn_c) (k_adjoint_source, geophone.hip) where a gradient call's
//                       residual kernel would put w_c (obs_c - syn_c), and Session::backward runs as in a gradient call: persistent loop
//                       or two-launch step, injection plans, the background's saved boundary frames.  Under a parameter file with if_win
//                       / filter (C = band-pass . window) the buffer gets -C^T Z C dsyn instead (Session::adjoint_source_conditioned):
//                       the product is J^T C^T Z C J v; the gathers handed out stay the raw ones.  Under if_envelope_misfit the product is
//                       J^T C^T D^T Z D C J v, D the derivative of the squared envelope at C of the BACKGROUND gather: one more sampler
//                       launch per step records that gather (record_background), only under the key.  Under robust_misfit
//                       the product is J^T C^T Z W Z C J v, W the IRLS weight psi / r of (C obs, C of the background gather): the same
//                       recording, and the shot's conditioned observed gather is acquired from the store and released with the shot
// and after the last shot the gradient finalisation writes hv.  The session's observed data (but for the read under robust_misfit), misfit,
// misfit parts and pseudo-Hessian state are neither read nor written.  Option quiet_skip is ignored for this call (the scattered field has no quiet maps).
// exact = true (sepfwi_adjoint_exact with v set): v is masked to Omega, the backward half is Session::backward_exact and the
// finalisation the exact one on Omega (exact_adjoint.hpp) -- the product P J^T W J P v, symmetric and non-negative.
// dStf (sepfwi_born_src, sepfwi_adjoint_exact_src): the scattered field takes a source term of its own (born.hpp, "Source block"), so the
// gathers are J_m v + J_s ds; v may be absent (the perturbed media are zeroed, k_born_media is not launched).  With exact and hv_stf the
// product has a fourth block, J_s^T W J u (Session::write_stf_exact).  Without dStf every launch and every bit is what it was.
#include <algorithm>
#include <cstring>
#include <vector>

#include "born.hpp"
#include "das_gauge.hpp"
#include "device_alloc.hpp"
#include "exact_adjoint.hpp"
#include "geophone.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "session.hpp"

namespace sepfwi {

// Axial-strain column `column` of the shot's BACKGROUND state into born_bg_ (time-major like the lane's own gathers): record_column
// with the one component and the one target.
void Session::record_background(const ShotCtx &x, int column) {
    float *col = born_bg_.get() + (size_t)column * x.nrec;
    if (x.gauge)
        launch_record_gauge(x.st, x.fld, x.nrec, x.rec, x.gauge->start.get(), x.gauge->cell.get(), x.gauge->field.get(), x.gauge->w.get(), nullptr, nullptr, nullptr,
                            col, 8);
    else
        launch_record(x.st, g_, x.fld, x.nrec, x.rec, nullptr, nullptr, nullptr, col, 8, x.sens);
    cs_.launches++;
}

void Session::born(float *d_ett, float *d_vx, float *d_vz, float *hv_Lambda, float *hv_Mu, float *hv_Den, const float *Lambda, const float *Mu,
                   const float *Den, const float *dLambda, const float *dMu, const float *dDen, const float *stf, int group_size, const int *shot_ids,
                   hipStream_t ext_stream, bool exact, const float *dStf, float *hv_stf) {
    std::lock_guard<std::mutex> lock(mu_);
    const bool want_hv = hv_Lambda != nullptr, have_v = dLambda != nullptr;
    // refusals first: nothing is touched
    const MisfitTraits &kind = traits(par_.misfit);
    if (want_hv && (!kind.gauss_newton || par_.if_src_update))
        throw std::invalid_argument(par_.misfit == Misfit::W2
            ? "born: the Gauss-Newton product is not defined under if_w2_misfit (the transport misfit has no least-squares form in the data); "
              "the scattered gathers alone are served (hv_* = NULL)"
            : "born: the Gauss-Newton product is not defined for a conditioned misfit with if_cross_misfit or if_src_update (not "
              "quadratic in the data); if_win and filter are served; the scattered gathers alone are served under every key (hv_* = NULL)");
    check_shot_ids(group_size, shot_ids);  // (begin_call checks them where run does: after it has touched the statistics)
    Call c = begin_call(ext_stream, group_size, shot_ids);
    c.opt.quiet_skip = 0;
    c.with_adj = want_hv;  // (if_res, to_store stay false: no observed data, no misfit, no files; the observed store is not touched --
                           // but for the product under robust_misfit, whose weight needs the shot's conditioned observed gather: below)
    hipStream_t st = c.st;
    last_batched_ = false;
    cs_.exact = exact && want_hv;

    prepare_media(c, Lambda, Mu, Den);  // (the Courant guard: the background model only)
    prepare_buffers(c, stf);

    const size_t n = cells_, dense = (size_t)par_.nz * (size_t)par_.nx;
    const int nSteps = par_.nSteps;
    if (!born_) born_ = dev<float>((kStateArrays + 5) * n);
    const float *dv[3] = {dLambda, dMu, dDen};
    for (int k = 0; k < 3 && have_v; k++) {
        if (!exact && ptr_device(dv[k]) == gpu_id_) continue;  // (the exact product reads v on Omega only: it masks a copy)
        if (!born_stage_) born_stage_ = dev<float>(3 * dense);
        HIP_OK(hipMemcpyAsync(born_stage_.get() + (size_t)k * dense, dv[k], dense * sizeof(float), hipMemcpyDefault, st));
        dv[k] = born_stage_.get() + (size_t)k * dense;
    }
    if (exact && have_v) {
        launch_exact_mask(st, g_, born_stage_.get(), 3, dense);
        cs_.launches++;
    }
    const float *mu_dense = ptr_device(Mu) == gpu_id_ ? Mu : in_stage_ + dense;  // (prepare_media staged it there)
    float *dstate = born_.get(), *dmedia = born_.get() + kStateArrays * n;  // [5 scattered fields | 8 memories] like a lane's state, then the media
    if (have_v) {
        launch_born_media(st, g_, mu_dense, dv[0], dv[1], dv[2], md_, dmedia, n);
        cs_.launches++;
    } else {  // the source block alone: the perturbed media are zero
        HIP_OK(hipMemsetAsync(dmedia, 0, 5 * n * sizeof(float), st));
    }
    // the perturbation of the source time function, row i the call's shot i: tapered like the source rows themselves (prepare_buffers)
    std::vector<float> ds_rows;
    if (dStf) {
        ds_rows.resize((size_t)group_size * nSteps);
        if (!ds_rows.empty()) HIP_OK(hipMemcpy(ds_rows.data(), dStf, ds_rows.size() * sizeof(float), hipMemcpyDefault));
        for (int i = 0; i < group_size; i++) stf_taper(ds_rows.data() + (size_t)i * nSteps, nSteps, par_.dt, 0.001f);
    }

    // which scattered gathers the call needs: the requested ones, and for the product the components with a weight
    int comps = (d_ett ? 8 : 0) | (d_vx ? 2 : 0) | (d_vz ? 4 : 0);
    if (want_hv) comps |= active_comps();
    // envelope misfit: the product linearises the envelope at the BACKGROUND gather, which the samplers record into a buffer of its own
    // robust misfit: the IRLS weight is taken at the background gather too, and at the shot's conditioned OBSERVED gather from the store
    const bool robust = want_hv && kind.needs_obs, bg = want_hv && kind.at_background;
    if (bg && !born_bg_) born_bg_ = dev<float>(data_len_);
    if (bg) ensure_data_scratch();
    if (robust) obs_begin(c);
    float *out[4] = {nullptr, d_vx, d_vz, d_ett};
    size_t out_off = 0;
    const BornArgs args{state_, dstate, media_, dmedia, pc_.a_z, n};
    for (int is = 0; is < group_size; is++) {
        ShotCtx x = make_ctx(c, is, stream_lane(0, st), false);
        x.scratch = false;
        x.comps = comps;
        if (robust) x.d_obs = x.obs_c[3] = obs_->acquire(x.id, x.nrec, st, 3);  // held until the shot's adjoint source is formed
        ShotCtx xd = x;  // the samplers' view: the scattered fields
        xd.fld = fields_at(dstate, n);

        HIP_OK(hipEventRecord(ev_[0], st));
        forward_init(x);  // background state, column 0 of the gathers
        HIP_OK(hipMemsetAsync(dstate, 0, kStateArrays * n * sizeof(float), st));
        if (bg && x.nrec > 0) HIP_OK(hipMemsetAsync(born_bg_.get(), 0, (size_t)x.nrec * sizeof(float), st));  // column 0, as forward_init
        for (int it = 0; it <= nSteps - 2; it++) {
            float *frame_t = want_hv ? x.frame + (size_t)it * 5 * (size_t)g_.frame_len : nullptr;
            const float amp = c.src_scale * x.stf_s[it] * par_.dt;
            const float damp = dStf ? c.src_scale * ds_rows[(size_t)is * nSteps + it] * par_.dt : 0.0f;  // (the expression of amp)
            launch_born_stress(st, g_, c.opt, args, frame_t, x.sh->z_src, x.sh->x_src, amp, dStf ? &damp : nullptr);
            launch_born_velocity(st, g_, c.opt, args);
            cs_.launches += 2;
            if (x.nrec > 0 && comps) record_column(xd, it + 1);
            if (bg && x.nrec > 0) record_background(x, it + 1);
        }
        HIP_OK(hipEventRecord(ev_[1], st));
        cs_.fwd_steps += (long long)(nSteps - 1);

        const size_t cnt = (size_t)x.nrec * nSteps;
        for (int k = 1; k <= 3 && cnt; k++) {
            if (!out[k]) continue;
            launch_transpose(st, syn_of(x, k), xpose_, nSteps, x.nrec);  // [it][rec] -> [rec][it]
            HIP_OK(hipMemcpyAsync(out[k] + out_off, xpose_, cnt * sizeof(float), hipMemcpyDefault, st));
            cs_.launches++;
        }
        out_off += cnt;
        if (want_hv && cond_on_) {  // if_win / filter: -C^T Z C J v (the weights are (1, 0, 0): the axial strain alone)
            adjoint_source_conditioned(c, x);
            if (robust) obs_->release_all();
        } else if (want_hv && x.nrec > 0) {
            AdjSource q{{}, {}, 1, (size_t)x.nrec, x.res, x.nrec, geo_ncomp_};  // the time-major gathers of J v, by the weights
            for_active([&](int comp, int b) {
                q.src[b] = syn_of(x, comp);
                q.scale[b] = par_.weight(comp);
            });
            launch_adjoint_source(st, q, nSteps);
            cs_.launches++;
        }
        cs_.fwd_ms += bracket_ms(0, st);  // (the time loop alone: ev_[1] was recorded before the gathers left)
        if (want_hv && exact)
            backward_exact(c, x, hv_stf != nullptr);
        else if (want_hv)
            backward(c, x);  // (a shot without channels: nothing is injected, as in a gradient call)
    }
    if (want_hv && exact) {
        write_outputs_exact(c, hv_Lambda, hv_Mu, hv_Den);
        if (hv_stf) write_stf_exact(c, hv_stf);
    } else if (want_hv)
        write_outputs(c, nullptr, hv_Lambda, hv_Mu, hv_Den, nullptr);
    end_call(c, true);
}

}  // namespace sepfwi
