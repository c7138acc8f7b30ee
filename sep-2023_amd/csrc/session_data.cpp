// session_data.cpp -- the data-conditioning chain of the misfit as the session composes it, and every way into it.
//
// The Conditioner (conditioning.hip) owns the kernels, the FFT work space and the count of what it issues; the session owns the [rec][it]
// scratch gathers xpose_, xpose2_, xpose3_ (one shot each: the chain runs on the call's MAIN stream, shot after shot) and the order of the
// stages, that of the reference's commented lines (libCUFD.cu:353-457) with the apparent-slowness fan filter across a shot's channels
// (fk_slowness / fk_mode, conditioning.hpp: fk_filter) as the third: C = FK . band-pass . window (condition_gather), C^T = window . band-pass . FK
// (condition_gather_t), and the two middles misfit_chain and gn_chain (session.hpp).  Inside a call the middles run between two
// transpositions of the shot's time-major gathers: residual_conditioned (run, adjoint_exact) and adjoint_source_conditioned (born); these
// charge their transpositions and what the Conditioner counted across the chain to sepfwi_stats.launches.  (The observed store conditions a
// gather when it is installed, obs_store.cpp: that is charged to no call.)
//
// The entry points take RAW axial-strain gathers, [nrec_i][nSteps] shot after shot like born()'s d_ett, host or device, with no propagation:
//   condition     sepfwi_condition: C or C^T in place
//   data_misfit   the file's misfit of (obs, syn) and the raw-space adjoint source a = -d misfit / d syn: C^T Z (C obs - C syn) under an L2
//                 file, the adjoint source of the normalised cross-correlation under if_cross_misfit, C^T D^T Z (e(C obs) - e(C syn)) under
//                 if_envelope_misfit, -1/2 C^T w dW / d(C syn) under if_w2_misfit (w2_misfit.hpp), C^T psi under robust_misfit
//                 (robust_misfit.hpp).  Under if_src_update the matching filter is computed from the call's own (C obs, C syn), shot by shot,
//                 as a gradient call computes it; the misfit is that of the updated synthetics and a is taken with the filter held fixed
//                 (nothing is carried from one shot or call to the next).
//   data_gn       the Gauss-Newton operator of the misfit in data space at syn: C^T Z C d, or C^T D^T Z D C d under if_envelope_misfit, or
//                 (sepfwi_data_gn_obs alone: the weight needs the observed data) C^T Z W Z C d under robust_misfit, W the IRLS weight of
//                 (C obs, C syn) (robust_misfit.hpp).  Refused where the products are: a kind without one (kMisfitTraits), if_src_update.
// A file without a live conditioning key has C = 1 and no conditioner: its misfit runs through the residual kernel of its gradient calls
// (time-major, lane 0's gather and residual buffers), its operator is Z.  A joint misfit (misfit_w_*) is refused: it is not one of axial
// strain alone.  The session's observed store, misfit, misfit parts and call statistics are neither read nor written; the callers' inputs
// are never changed.
#include <string>

#include "device_alloc.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "session.hpp"

namespace sepfwi {

// the window stage of a shot (libCUFD.cu:353-374)
void Session::window_gather(hipStream_t st, float *gather, int shot_id, int nrec) {
    const size_t tot = (size_t)rec_off_.back() + 1, off = (size_t)rec_off_[shot_id];
    const float *w = par_.if_win ? win_ + off : nullptr;  // [start | end | weight] per channel
    cond_->window(st, gather, nrec, par_.dt, w, w ? w + tot : nullptr, w ? w + 2 * tot : nullptr, w ? survey_.shots[shot_id].src_weight : 1.0f, 0.005f);
}

// Window and band-pass one [rec][it] gather in place, as the commented driver lines apply them to observed and synthetic
// data alike (libCUFD.cu:353-374); then the fan filter across the shot's channels (fk_slowness; no counterpart in the reference) at the
// shot's own channel spacing.  The stages are composed, not fused: band-pass and fan filter do not commute exactly (the crop between them).
void Session::condition_gather(hipStream_t st, float *gather, int shot_id, int nrec) {
    window_gather(st, gather, shot_id, nrec);
    if (par_.has_filter) cond_->bandpass(st, gather, nrec, par_.dt, par_.filter);
    if (par_.has_fk) cond_->fk_filter(st, gather, nrec, par_.dt, fk_delta_[shot_id], par_.fk_slowness, par_.fk_reject);
}

// Its transpose, as the commented lines apply it to the residual (libCUFD.cu:436-457): the (symmetric) fan filter first, the (zero-phase,
// symmetric) filter, then the (pointwise) window.
void Session::condition_gather_t(hipStream_t st, float *gather, int shot_id, int nrec) {
    if (par_.has_fk) cond_->fk_filter(st, gather, nrec, par_.dt, fk_delta_[shot_id], par_.fk_slowness, par_.fk_reject);
    if (par_.has_filter) cond_->bandpass(st, gather, nrec, par_.dt, par_.filter);
    window_gather(st, gather, shot_id, nrec);
}

void Session::misfit_chain(hipStream_t st, const float *obs_c, float *syn, float *out, int shot_id, int nrec, double *acc) {
    const size_t tot = (size_t)rec_off_.back() + 1, off = (size_t)rec_off_[shot_id];
    const Shot &sh = survey_.shots[shot_id];
    // the trace weights of the kinds that take them explicitly (Cross; W2: the window's amplitude cancels in the densities).  They belong to
    // if_win, as the window's do: without the key w_r = 1 (oracle.conditioned_residual)
    const float *tw = traits(par_.misfit).trace_weights && par_.if_win ? win_ + 2 * tot + off : nullptr;
    condition_gather(st, syn, shot_id, nrec);
    if (par_.if_src_update) cond_->source_update(st, obs_c, syn, nrec, par_.dt);  // libCUFD.cu:383-390
    switch (par_.misfit) {
        case Misfit::L2: cond_->l2_residual(st, obs_c, syn, out, nrec, acc); break;
        case Misfit::Cross: cond_->cross_residual(st, obs_c, syn, out, nrec, tw, sh.src_weight, acc); break;
        case Misfit::Envelope: cond_->envelope_residual(st, obs_c, syn, out, nrec, acc); break;  // rho = Z (e(C obs) - e(C syn)); D^T rho
        case Misfit::W2: cond_->w2_residual(st, obs_c, syn, out, nrec, tw, sh.src_weight, par_.dt, par_.w2_beta, acc); break;
        case Misfit::Robust:  // psi of the Huber / Cauchy penalty, the threshold from the conditioned observed trace (robust_misfit.hpp)
            cond_->robust_residual(st, obs_c, syn, out, nrec, par_.robust_kind, par_.robust_delta, par_.robust_quantile, acc);
            break;
    }
    if (par_.if_src_update) cond_->source_update_adj(st, out, nrec, par_.dt);  // libCUFD.cu:430-433
    condition_gather_t(st, out, shot_id, nrec);
}

void Session::gn_chain(hipStream_t st, float *d, float *bg, float *out, int shot_id, int nrec, float sign, const float *obs_c) {
    condition_gather(st, d, shot_id, nrec);
    if (traits(par_.misfit).at_background) condition_gather(st, bg, shot_id, nrec);
    switch (par_.misfit) {
        case Misfit::Cross: case Misfit::W2:  // (no Gauss-Newton product: every caller has refused)
        case Misfit::L2: cond_->scattered_residual(st, d, out, nrec, sign); break;
        case Misfit::Envelope: cond_->envelope_scattered(st, bg, d, out, nrec, sign); break;
        case Misfit::Robust:  // W = psi / r at the background: the IRLS weight of (C obs, C bg)
            cond_->robust_scattered(st, obs_c, bg, d, out, nrec, par_.robust_kind, par_.robust_delta, par_.robust_quantile, sign);
            break;
    }
    condition_gather_t(st, out, shot_id, nrec);
}

// residual + misfit of the axial-strain component with the chain (libCUFD.cu:353-457 as its commented lines compose it)
void Session::residual_conditioned(const Call &c, const ShotCtx &x) {
    if (x.nrec <= 0) return;
    hipStream_t st = c.st;
    const int nSteps = par_.nSteps;
    const long long before = cond_->launches();
    launch_transpose(st, syn_of(x, 3), xpose_, nSteps, x.nrec);  // [it][rec] -> [rec][it]
    misfit_chain(st, x.d_obs, xpose_, xpose2_, x.id, x.nrec, scal_);
    launch_transpose(st, xpose2_, x.res, x.nrec, nSteps);  // [rec][it] -> [it][rec]: the adjoint source
    cs_.launches += 2 + (cond_->launches() - before);
}

// The adjoint source of a Gauss-Newton product under a file whose live conditioning keys are if_win / filter: from the shot's
// scattered axial-strain gather d = J v (time-major, where the samplers left it) the residual buffer gets -C^T Z C d -- what
// residual_conditioned leaves for observed data syn - J v, and the sign k_adjoint_source leaves.  Z (sample 0 zeroed) and the sign
// are one kernel, in the place of the residual kernel; no misfit, no observed data.
// Under if_envelope_misfit the buffer gets -C^T D^T Z D C d, D the derivative of the squared envelope at C of the shot's BACKGROUND
// gather, which Session::born recorded time-major in born_bg_.  Under robust_misfit it gets -C^T Z W Z C d, W the IRLS weight of the
// shot's conditioned observed gather (x.d_obs, which Session::born acquired from the store) and C of the same recorded background gather.
void Session::adjoint_source_conditioned(const Call &c, const ShotCtx &x) {
    if (x.nrec <= 0) return;
    hipStream_t st = c.st;
    const bool bg = traits(par_.misfit).at_background;
    const long long before = cond_->launches();
    if (bg) launch_transpose(st, born_bg_.get(), xpose3_.get(), par_.nSteps, x.nrec);
    launch_transpose(st, syn_of(x, 3), xpose_, par_.nSteps, x.nrec);  // [it][rec] -> [rec][it]
    gn_chain(st, xpose_, bg ? xpose3_.get() : nullptr, xpose2_, x.id, x.nrec, -1.0f, x.d_obs);
    launch_transpose(st, xpose2_, x.res, x.nrec, par_.nSteps);  // [rec][it] -> [it][rec]
    cs_.launches += (bg ? 3 : 2) + (cond_->launches() - before);
}

// the third [rec][it] scratch gather and the sum of the data-space entry points (and of the envelope product of Session::born)
void Session::ensure_data_scratch() {
    if (!xpose3_) xpose3_ = dev<float>(data_len_);
    if (!data_acc_) data_acc_ = dev<double>(1);
}

// ---- the entry points on the caller's gathers: each holds the lock and makes its refusals first ----
hipStream_t Session::data_stream(hipStream_t ext_stream) {
    HIP_OK(hipSetDevice(gpu_id_));
    hipStream_t st = ext_stream ? ext_stream : own_stream_.get();
    if (!ext_stream) order_after_null_stream(st);
    return st;
}

// f(shot id, nrec, offset of the shot's gather in the caller's arrays, its length), shots without channels skipped
template <class F> void Session::for_each_gather(int group_size, const int *shot_ids, F f) {
    size_t off = 0;
    for (int is = 0; is < group_size; is++) {
        const int id = shot_ids[is], nrec = survey_.shots[id].nrec;
        const size_t cnt = (size_t)nrec * par_.nSteps;
        if (cnt == 0) continue;
        f(id, nrec, off, cnt);
        off += cnt;
    }
}

// A gather on this device is conditioned where it lies, any other one in the session's scratch gather.
void Session::condition(float *data, bool transpose, int group_size, const int *shot_ids, hipStream_t ext_stream) {
    std::lock_guard<std::mutex> lock(mu_);
    check_shot_ids(group_size, shot_ids);
    if (!cond_on_) return;  // the identity
    hipStream_t st = data_stream(ext_stream);
    for_each_gather(group_size, shot_ids, [&](int id, int nrec, size_t off, size_t cnt) {
        float *g = data + off;
        const bool staged = ptr_device(g) != gpu_id_;
        if (staged) {
            HIP_OK(hipMemcpyAsync(xpose_, g, cnt * sizeof(float), hipMemcpyDefault, st));
            g = xpose_;
        }
        transpose ? condition_gather_t(st, g, id, nrec) : condition_gather(st, g, id, nrec);
        if (staged) HIP_OK(hipMemcpyAsync(data + off, xpose_, cnt * sizeof(float), hipMemcpyDefault, st));
    });
    HIP_OK(hipStreamSynchronize(st));
}

void Session::data_misfit(float *misfit, float *adj, const float *obs, const float *syn, int group_size, const int *shot_ids, hipStream_t ext_stream) {
    std::lock_guard<std::mutex> lock(mu_);
    if (joint_) throw std::invalid_argument("data_misfit: not defined for a joint misfit (misfit_w_*): it is a misfit of axial-strain gathers alone");
    check_shot_ids(group_size, shot_ids);
    hipStream_t st = data_stream(ext_stream);
    ensure_data_scratch();
    double *acc = data_acc_.get();
    HIP_OK(hipMemsetAsync(acc, 0, sizeof(double), st));
    const int nSteps = par_.nSteps;
    for_each_gather(group_size, shot_ids, [&](int id, int nrec, size_t off, size_t cnt) {
        const size_t bytes = cnt * sizeof(float);
        if (cond_on_) {  // the observed gather is kept conditioned (obs_store.cpp): C obs, then the chain on the raw synthetic gather
            HIP_OK(hipMemcpyAsync(xpose3_.get(), obs + off, bytes, hipMemcpyDefault, st));
            condition_gather(st, xpose3_.get(), id, nrec);
            HIP_OK(hipMemcpyAsync(xpose_, syn + off, bytes, hipMemcpyDefault, st));
            misfit_chain(st, xpose3_.get(), xpose_, xpose2_, id, nrec, acc);
            if (adj) HIP_OK(hipMemcpyAsync(adj + off, xpose2_, bytes, hipMemcpyDefault, st));
        } else {  // the plain residual kernel of a gradient call, on time-major gathers: lane 0's gather and residual buffers
            float *t_obs = syn_, *t_syn = syn_ + data_len_;
            HIP_OK(hipMemcpyAsync(xpose_, obs + off, bytes, hipMemcpyDefault, st));
            launch_transpose(st, xpose_, t_obs, nrec, nSteps);  // [rec][it] -> [it][rec]
            HIP_OK(hipMemcpyAsync(xpose_, syn + off, bytes, hipMemcpyDefault, st));
            launch_transpose(st, xpose_, t_syn, nrec, nSteps);
            launch_residual(st, t_obs, t_syn, res_, nrec, (long long)cnt, acc);
            launch_transpose(st, res_, xpose_, nSteps, nrec);  // [it][rec] -> [rec][it]
            if (adj) HIP_OK(hipMemcpyAsync(adj + off, xpose_, bytes, hipMemcpyDefault, st));
        }
    });
    double sum = 0.0;
    HIP_OK(hipMemcpyAsync(&sum, acc, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const float mf = (float)(0.5 * sum);  // as read_misfit halves the total
    if (misfit) HIP_OK(hipMemcpy(misfit, &mf, sizeof(float), hipMemcpyDefault));
}

void Session::data_gn(float *out, const float *obs, const float *syn, const float *d, int group_size, const int *shot_ids, hipStream_t ext_stream,
                      bool obs_entry) {
    std::lock_guard<std::mutex> lock(mu_);
    const MisfitTraits &kind = traits(par_.misfit);
    const bool robust = kind.needs_obs, env = kind.at_background;  // env: the kinds whose operator depends on syn
    if (robust && !obs_entry)
        throw std::invalid_argument("data_gn: under robust_misfit the operator's weight needs the observed data; call sepfwi_data_gn_obs(out, obs, syn, d, ...)");
    if (robust && !obs && group_size > 0) throw std::invalid_argument("data_gn_obs: obs must not be NULL under robust_misfit (the weight is formed from C obs - C syn)");
    if (!kind.gauss_newton || par_.if_src_update)  // (if_src_update stands beside no kind without the product: parse_params, the constructor)
        throw std::invalid_argument(std::string("data_gn: not defined under ") + (par_.if_src_update ? "if_src_update" : kind.key) +
                                    " (not a least-squares misfit of the data); if_win, filter and if_envelope_misfit are served");
    if (joint_) throw std::invalid_argument("data_gn: not defined for a joint misfit (misfit_w_*): it is a misfit of axial-strain gathers alone");
    check_shot_ids(group_size, shot_ids);
    hipStream_t st = data_stream(ext_stream);
    if (env) ensure_data_scratch();
    float *obs_c = robust ? syn_ : nullptr;  // a fourth [rec][it] gather: lane 0's gather buffers, as data_misfit borrows them under a plain file
    for_each_gather(group_size, shot_ids, [&](int id, int nrec, size_t off, size_t cnt) {
        const size_t bytes = cnt * sizeof(float);
        HIP_OK(hipMemcpyAsync(xpose_, d + off, bytes, hipMemcpyDefault, st));
        if (cond_on_) {
            if (env) HIP_OK(hipMemcpyAsync(xpose3_.get(), syn + off, bytes, hipMemcpyDefault, st));
            if (robust) {
                HIP_OK(hipMemcpyAsync(obs_c, obs + off, bytes, hipMemcpyDefault, st));
                condition_gather(st, obs_c, id, nrec);
            }
            gn_chain(st, xpose_, env ? xpose3_.get() : nullptr, xpose2_, id, nrec, 1.0f, obs_c);
            HIP_OK(hipMemcpyAsync(out + off, xpose2_, bytes, hipMemcpyDefault, st));
        } else {  // Z alone: sample 0 of every trace zeroed
            HIP_OK(hipMemset2DAsync(xpose_, (size_t)par_.nSteps * sizeof(float), 0, sizeof(float), (size_t)nrec, st));
            HIP_OK(hipMemcpyAsync(out + off, xpose_, bytes, hipMemcpyDefault, st));
        }
    });
    HIP_OK(hipStreamSynchronize(st));
}

}  // namespace sepfwi
