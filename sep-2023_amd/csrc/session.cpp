// session.cpp -- persistent per-(parameter file, GPU) propagation session and the cufd driver.
//
// Replaces the per-call host driver of the reference, Src/libCUFD.cu:32-820 (set-up :39-165, shot loop
// :170-708, gradient read-back :710-724, seismogram files :755-769) and the classes it instantiates on
// every call: Model (Src/Model.cu), Cpml (Src/Cpml.cu), Bnd (Src/Boundary.cu), Src_Rec (Src/Src_Rec.cu).
// Differences by design: device state is allocated once and kept; observed data are cached
// in HBM (time-major) instead of being re-read from four files per shot per call; only the axial-strain
// (ett) residual -- the only one that enters misfit and adjoint source (libCUFD.cu:427,607) -- is formed, unless the
// parameter keys misfit_w_* give the vx / vz residuals a weight (geophone.hpp).
#include "session.hpp"

#include <sys/stat.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>

#include "das_gauge.hpp"
#include "geophone.hpp"
#include "device_alloc.hpp"
#include "hip_check.hpp"
#include "host_checks.hpp"
#include "kernels.hpp"

namespace sepfwi {

template <class T>
T *Session::dalloc(size_t n) {
    allocs_.push_back(dev<char>(n * sizeof(T)));
    return (T *)allocs_.back().get();
}

// grid geometry of the session from the parameter file (Parameter.cpp:41-178, Boundary.cu:17-27)
void Session::init_grid() {
    const Params &par = par_;
    Grid &g = g_;
    g.nz = par.nz;
    g.nx = par.nx;
    g.nzc = par.nz - par.nPad;
    g.pitch = ((par.nx + 63) / 64) * 64;
    g.fiber = par.fiber;
    g.nPml = par.nPml;
    g.zmax = g.nzc - 1 - par.nPml;
    g.xmax = par.nx - 1 - par.nPml;
    g.nSteps = par.nSteps;
    g.dt = par.dt;
    g.dt_img = par.dt;
    g.dz = par.dz;
    g.dx = par.dx;
    g.rdz = 1.0f / par.dz;
    g.rdx = 1.0f / par.dx;
    g.nzBnd = g.nzc - 2 * par.nPml + 4;  // Boundary.cu:17-18
    g.nxBnd = par.nx - 2 * par.nPml + 4;
    g.frame_len = 10 * g.nxBnd + 10 * (g.nzBnd - 10);
    g.qzw = ((g.nzc + 4) >> 5) + 2;          // quiet-segment maps (Fields::q): bits z + 2 of rows -2 ... nzc + 1, one spare word for the 64-bit window
    g.qn = (g.pitch / 64 + 2) * g.qzw;        // segment columns -1 ... pitch / 64

}

// [5 fields | 8 C-PML memories | 5 adjoint fields] contiguous (one memset clears a group; the fused kernels take them as bundles),
// media, accumulators, staging for foreign-memory inputs / outputs (libCUFD.cu:127-146)
void Session::alloc_arrays() {
    const Params &par = par_;
    const Grid &g = g_;
    const size_t n = (size_t)(g.nzc + 4) * (size_t)g.pitch;  // 4 spare rows
    cells_ = n;
    state_ = dalloc<float>(kOwnArrays * n);
    fld_ = fields_at(state_, n);
    mem_ = mem_at(state_mem(state_, n), n);
    adj_ = fields_at(own_adj(state_, n), n);
    media_ = dalloc<float>(6 * n);
    HIP_OK(hipMemset(media_, 0, 6 * n * sizeof(float)));
    HIP_OK(hipDeviceSynchronize());  // the fill runs on the null stream and does not block the host; a caller's non-blocking stream would not wait for it
    md_ = media_at(media_, n);
    acc_buf_ = dalloc<float>(kAccArrays * n);
    quiet_pool_ = dalloc<unsigned int>((size_t)kQuietSlots * 4 * (size_t)g.qn);
    acc_ = acc_at(acc_buf_, n);
    const size_t dense = (size_t)par.nz * (size_t)par.nx;
    in_stage_ = dalloc<float>(3 * dense);
    grad_stage_ = dalloc<float>(3 * dense);
    scal_ = dalloc<double>(4);
    cp2_bits_ = dalloc<unsigned int>(4);

}

// C-PML profiles (host) -> device, with 1/K precomputed (Cpml.cu:7-117, utilities.cu:243-359)
void Session::upload_profiles() {
    const Params &par = par_;
    const Grid &g = g_;
    {
        const int nzc = g.nzc, nx = g.nx;
        std::vector<float> K(std::max(nzc, nx)), a(K.size()), b(K.size()), Kh(K.size()), ah(K.size()), bh(K.size());
        std::vector<float> hz(6 * (size_t)nzc), hx(6 * (size_t)nx);
        cpml_profiles(K.data(), a.data(), b.data(), Kh.data(), ah.data(), bh.data(), nzc, par.nPml, par.dz, par.f0, par.dt);
        for (int i = 0; i < nzc; i++) {
            hz[i] = a[i]; hz[nzc + i] = b[i]; hz[2 * nzc + i] = 1.0f / K[i];
            hz[3 * nzc + i] = ah[i]; hz[4 * nzc + i] = bh[i]; hz[5 * nzc + i] = 1.0f / Kh[i];
        }
        cpml_profiles(K.data(), a.data(), b.data(), Kh.data(), ah.data(), bh.data(), nx, par.nPml, par.dx, par.f0, par.dt);
        for (int i = 0; i < nx; i++) {
            hx[i] = a[i]; hx[nx + i] = b[i]; hx[2 * nx + i] = 1.0f / K[i];
            hx[3 * nx + i] = ah[i]; hx[4 * nx + i] = bh[i]; hx[5 * nx + i] = 1.0f / Kh[i];
        }
        float *dz_ = dalloc<float>(hz.size() + hx.size()), *dx_ = dz_ + hz.size();  // contiguous: kernels may address x profiles as z base + 6*nzc
        HIP_OK(hipMemcpy(dz_, hz.data(), hz.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dx_, hx.data(), hx.size() * sizeof(float), hipMemcpyHostToDevice));
        pc_ = PmlCoef{dz_, dz_ + nzc, dz_ + 2 * nzc, dz_ + 3 * nzc, dz_ + 4 * nzc, dz_ + 5 * nzc,
                      dx_, dx_ + nx,  dx_ + 2 * nx,  dx_ + 3 * nx,  dx_ + 4 * nx,  dx_ + 5 * nx};
    }

}

// receivers: flat cell index per shot (validated against the grid: host_checks.cpp), directional sensitivities, per-channel windows
void Session::upload_survey() {
    const Grid &g = g_;
    {
        const int ns = (int)survey_.shots.size();
        std::vector<int> idx;
        receiver_cells(par_, survey_, g.nzc, g.nx, g.pitch, &rec_off_, &idx);
        check_gauge_members(par_, survey_, g.nzc, g.nx);  // parameter key das_gauge_length: every member of a gauge where a channel may lie
        rec_idx_ = dalloc<int>(idx.size());
        HIP_OK(hipMemcpy(rec_idx_, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
        bool any_sens = false;
        for (int i = 0; i < ns; i++) any_sens = any_sens || (survey_.shots[i].present && !survey_.shots[i].sens.empty());
        if (any_sens) {  // (s_xx, s_zz, s_xz) per channel, same offsets as rec_idx_
            std::vector<float> sv(3 * idx.size(), 0.0f);
            for (int i = 0; i < ns; i++) {
                const Shot &sh = survey_.shots[i];
                if (sh.present && !sh.sens.empty()) std::copy(sh.sens.begin(), sh.sens.end(), sv.begin() + 3 * (size_t)rec_off_[i]);
            }
            sens_ = dalloc<float>(sv.size());
            HIP_OK(hipMemcpy(sens_, sv.data(), sv.size() * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    if (cond_on_) {  // [start | end | weight] per channel, read under if_win alone (the windows, and the trace weights of the cross-correlation misfit)
        const int ns = (int)survey_.shots.size();
        const size_t tot = (size_t)rec_off_[ns] + 1;
        std::vector<float> w(3 * tot, 0.0f);
        for (int i = 0; i < ns; i++) {
            const Shot &sh = survey_.shots[i];
            if (!sh.present) continue;
            for (int r = 0; r < sh.nrec; r++) {
                const size_t k = (size_t)rec_off_[i] + r;
                w[k] = sh.win_start.empty() ? 0.0f : sh.win_start[r];
                w[tot + k] = sh.win_end.empty() ? 0.0f : sh.win_end[r];
                w[2 * tot + k] = sh.weights.empty() ? 1.0f : sh.weights[r];
            }
        }
        win_ = dalloc<float>(w.size());
        HIP_OK(hipMemcpy(win_, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    }
}

Session::Session(const std::string &para_fname, int gpu_id, const std::string &para_text,
                 const std::string &survey_text, const Params &par, const Survey &survey)
    : para_fname_(para_fname), gpu_id_(gpu_id), para_text_(para_text), survey_text_(survey_text), par_(par),
      survey_(survey) {
    // The data-conditioning keys are dormant in the reference (every call site is commented out, libCUFD.cu:353-457; the one live
    // line, source_update_adj at :430-433, acts on the pressure residual that is never injected).  Here a key switches its
    // stage on for the axial-strain gathers (conditioning.hip).  One combination has no defined meaning there either: the
    // commented lines take the trace norms of the cross-correlation misfit BEFORE the source update and use them after it.
    if (par.if_src_update && par.misfit == Misfit::Cross)
        throw std::invalid_argument("parameter file: if_src_update together with if_cross_misfit is not supported");
    cond_on_ = par.first_live_key() != nullptr;
    if (par.has_fk) fk_channel_spacing(par_, survey_, &fk_delta_);  // refuses a survey whose channels are no straight, equally spaced line: before anything is allocated
    joint_ = par.joint();
    geo_ncomp_ = geo_blocks(par, geo_block_);
    HIP_OK(hipSetDevice(gpu_id_));
    own_stream_ = make_stream();
    ev_order_ = make_event(false);
    for (auto &e : ev_) e = make_event(true);
    for (auto &e : probe_ev_) e = make_event(true);

    init_grid();
    alloc_arrays();
    upload_profiles();
    upload_survey();
    const size_t dlen = (size_t)std::max(1, survey_.max_nrec) * (size_t)par.nSteps;
    data_len_ = dlen;
    syn_ = dalloc<float>(4 * dlen);  // time-major pr, vx, vz, ett
    res_len_ = dlen * (size_t)(joint_ ? geo_ncomp_ : 1);  // today's size unless the misfit is a joint one
    res_ = dalloc<float>(res_len_);
    if (joint_) geo_sums_ = dalloc<double>(4);
    xpose_ = dalloc<float>(dlen);
    if (cond_on_) {
        xpose2_ = dalloc<float>(dlen);
        cond_.reset(new Conditioner(par.nSteps, std::max(1, survey_.max_nrec)));
        if (par.if_src_update) cond_->ensure_source_buffers(own_stream_);  // now: no shot pays an allocation inside its time loop
        switch (par.misfit) {
            case Misfit::L2: case Misfit::Cross: break;
            case Misfit::Envelope: cond_->ensure_envelope_buffers(); break;
            case Misfit::W2: cond_->ensure_w2_buffers(); break;
            case Misfit::Robust: cond_->ensure_robust_buffers(); break;
        }
        if (par.has_fk) cond_->ensure_fk_buffers();
    }
    h_io_.ensure(dlen);
    {
        ObservedStore::Host h;
        h.gpu_id = gpu_id_;
        h.par = &par_;
        h.survey = &survey_;
        h.xpose = xpose_;
        h.h_io = h_io_.get();
        h.cond_on = cond_on_;
        h.condition = [this](hipStream_t st, float *gather, int shot_id, int nrec) { condition_gather(st, gather, shot_id, nrec); };
        obs_.reset(new ObservedStore(h));
    }
    // everything the constructor put on the null stream (fills, profile / receiver tables copied from pageable host memory) is
    // complete before any stream of a later call -- the session's own non-blocking ones or a caller's -- can touch it
    HIP_OK(hipDeviceSynchronize());
}

// The members free what they own (session.hpp: buffers before events and streams); what is left to do is to let the device finish.
Session::~Session() {
    (void)hipSetDevice(gpu_id_);
    (void)hipDeviceSynchronize();
}

void Session::ensure_lane_stream(XLane &L) {
    if (L.stream) return;
    L.stream = make_stream();
    L.join = make_event(false);
}

// Extra lanes of forward state (fields, memory variables, boundary frames, seismograms, residual) and their streams.
void Session::ensure_lanes(int n_lanes, bool with_frames) {
    const size_t n = cells_;
    for (int k = 1; k < n_lanes && k < kMaxLanes; k++) {
        XLane &L = xl_[k];
        ensure_lane_stream(L);
        if (!L.state) {
            L.state = dev<float>(kStateArrays * n);
            L.syn = dev<float>(4 * data_len_);
            L.res = dev<float>(res_len_);
        }
        if (with_frames && !L.frame) L.frame = dev<float>(frame_lane_len());
    }
}

Session::Lane Session::stream_lane(int k, hipStream_t call_st) const {
    if (k == 0) return Lane{state_, frame_.get(), syn_, res_, quiet_slot(0), call_st};
    if (k < 0 || k >= kMaxLanes) return Lane{};
    const XLane &L = xl_[k];
    return Lane{L.state.get(), L.frame.get(), L.syn.get(), L.res.get(), quiet_slot(k), L.stream.get()};
}

Session::Lane Session::batch_lane(int k, hipStream_t call_st) const {
    const size_t n = cells_, j = (size_t)k;
    if (k < 0 || j >= ba_.state.size() / (kStateArrays * n)) return Lane{};
    float *frame = j < ba_.frame.size() / frame_lane_len() ? ba_.frame.get() + j * frame_lane_len() : nullptr;
    return Lane{ba_.state.get() + j * kStateArrays * n, frame, ba_.syn.get() + j * 4 * data_len_, ba_.res.get() + j * res_len_, quiet_slot(kMaxLanes + k), call_st};
}

float *Session::batch_bwd(int k) const {
    const size_t n = cells_, j = (size_t)k;
    return k >= 0 && j < ba_.bwd.size() / (kBwdArrays * n) ? ba_.bwd.get() + j * kBwdArrays * n : nullptr;
}

// Batched mode: n_fwd lanes of forward state, the first n_bwd of them with backward state too; shot table and source rows
// for n_shots shots.
// Lanes of the batched schedule.  The lanes of one kind lie in ONE arena at a constant stride (the multi-shot persistent loop
// addresses shot k of a launch as base + k stride, fwi_types.hpp MultiShot); an arena that is too small is replaced -- lanes carry
// nothing from one call to the next.
void Session::ensure_batch(int n_fwd, int n_bwd, bool with_frames, int n_shots) {
    const size_t n = cells_;
    ba_.state.ensure((size_t)n_fwd * kStateArrays * n);
    ba_.syn.ensure((size_t)n_fwd * 4 * data_len_);
    ba_.res.ensure((size_t)n_fwd * res_len_);
    if (with_frames) ba_.frame.ensure((size_t)n_fwd * frame_lane_len());
    ba_.bwd.ensure((size_t)n_bwd * kBwdArrays * n);
    d_shots_.ensure((size_t)n_shots);
    d_stf_.ensure((size_t)n_shots * par_.nSteps);
}

void Session::drop_observed() {
    std::lock_guard<std::mutex> lock(mu_);
    (void)hipSetDevice(gpu_id_);
    obs_->clear();
}

// Observed gather of one shot and component handed over from memory ([nrec][nSteps], host or device pointer).
void Session::set_observed(int shot_id, const float *ett, int nrec, int nSteps, int comp) {
    std::lock_guard<std::mutex> lock(mu_);
    HIP_OK(hipSetDevice(gpu_id_));
    if (comp < 1 || comp > 3) throw std::invalid_argument("set_observed: comp must be 1 (vx), 2 (vz) or 3 (ett), got " + std::to_string(comp));
    if (shot_id < 0 || shot_id >= (int)survey_.shots.size() || !survey_.shots[shot_id].present)
        throw std::invalid_argument("set_observed: unknown shot id " + std::to_string(shot_id));
    if (!ett || nrec != survey_.shots[shot_id].nrec || nSteps != par_.nSteps)
        throw std::invalid_argument("set_observed: data must be [nrec][nSteps] of the survey / parameter file");
    if (nrec > 0) order_after_null_stream(own_stream_);  // a HIP `ett` was produced on the caller's (default) stream
    obs_->release_all();
    obs_->put(shot_id, ett, nrec, own_stream_, comp);
}

void Session::misfit_parts(double parts[3]) {
    std::lock_guard<std::mutex> lock(mu_);
    for (int k = 0; k < 3; k++) parts[k] = parts_[k];
}

// Test hook (sepfwi_debug_field): one wavefield of one forward lane as the last call left it, dense (nzc, nx).
void Session::copy_field(int lane, int which, float *out) {
    std::lock_guard<std::mutex> lock(mu_);
    HIP_OK(hipSetDevice(gpu_id_));
    if (!out || which < 0 || which > 14) throw std::invalid_argument("debug_field: which must be 0..14");
    const float *base = nullptr;
    if (which >= 10) {  // the scattered fields of the last Born call
        if (!born_) throw std::invalid_argument("debug_field: no Born call yet");
        base = born_.get() + (size_t)(which - 10) * cells_;
    } else if (which >= 5) {  // adjoint fields: one set per session (stream mode) or per backward lane (batched mode)
        const float *adj = last_batched_ ? (batch_bwd(lane) ? bwd_adj(batch_bwd(lane), cells_) : nullptr) : adj_.vz;
        if (!adj) throw std::invalid_argument("debug_field: no such backward lane");
        base = adj + (size_t)(which - 5) * cells_;
    } else {
        const Lane L = last_batched_ ? batch_lane(lane) : stream_lane(lane);
        if (!L.state) throw std::invalid_argument("debug_field: no such lane");
        base = L.state + (size_t)which * cells_;
    }
    HIP_OK(hipMemcpy2D(out, (size_t)g_.nx * sizeof(float), base, (size_t)g_.pitch * sizeof(float), (size_t)g_.nx * sizeof(float),
                       (size_t)g_.nzc, hipMemcpyDefault));
}

void Session::stats(sepfwi_stats *out) const {
    out->fwd_ms = cs_.fwd_ms;
    out->bwd_ms = cs_.bwd_ms;
    out->total_ms = total_ms_;
    out->n_c = g_.nzc * g_.nx;
    out->fwd_steps = cs_.fwd_steps;
    out->bwd_steps = cs_.bwd_steps;
    out->launches = cs_.launches;
    out->device_bytes = device_bytes_ + (cond_ ? cond_->device_bytes() : 0) + obs_->device_bytes();
    out->obs_device_bytes = obs_->device_bytes();
    out->obs_host_bytes = obs_->host_bytes();
    out->obs_evictions = obs_->evictions();
    out->persist_steps = cs_.persist_steps;
    out->quiet_active = cs_.quiet_active;
    out->quiet_total = cs_.quiet_total;
    out->probe_kernel_us = cs_.probe_calls ? cs_.probe_us / (double)cs_.probe_calls : 0.0;
    out->probe_calls = cs_.probe_calls;
    // one forward pass = N_c*(nSteps-1); fwd+adj = 3x (forward, reconstruction, adjoint)
    out->cell_updates = (double)out->n_c * ((double)cs_.fwd_steps + 2.0 * (double)cs_.bwd_steps);
}

// ------------------------------------------------------------------------------------------------
// registry
// ------------------------------------------------------------------------------------------------
static std::mutex g_reg_mu;
static std::map<std::pair<std::string, int>, std::shared_ptr<Session>> g_sessions;

std::shared_ptr<Session> get_session(const std::string &para_fname, int gpu_id) {
    const std::string ptext = read_first_line(para_fname);
    Params par = parse_params(ptext);
    const std::string stext = read_first_line(par.survey_fname);
    std::lock_guard<std::mutex> lock(g_reg_mu);
    auto key = std::make_pair(para_fname, gpu_id);
    auto it = g_sessions.find(key);
    if (it != g_sessions.end() && it->second->matches(ptext, stext)) return it->second;
    if (it != g_sessions.end()) g_sessions.erase(it);  // a thread still inside run() keeps its own reference
    Survey sv = parse_survey(stext, par.nPml, par.if_win_key);
    int ndev = 0;
    HIP_OK(hipGetDeviceCount(&ndev));
    if (gpu_id < 0 || gpu_id >= ndev)
        throw HipError("gpu_id " + std::to_string(gpu_id) + " out of range: " + std::to_string(ndev) + " HIP device(s) visible");
    auto sp = std::make_shared<Session>(para_fname, gpu_id, ptext, stext, par, sv);
    g_sessions[key] = sp;
    return sp;
}

std::shared_ptr<Session> find_session(const std::string &para_fname, int gpu_id) {
    std::lock_guard<std::mutex> lock(g_reg_mu);
    auto it = g_sessions.find(std::make_pair(para_fname, gpu_id));
    return it == g_sessions.end() ? nullptr : it->second;
}

void release_all_sessions() {
    std::lock_guard<std::mutex> lock(g_reg_mu);
    g_sessions.clear();
}

void invalidate_observed_all() {
    std::vector<std::shared_ptr<Session>> all;
    {
        std::lock_guard<std::mutex> lock(g_reg_mu);
        for (auto &kv : g_sessions) all.push_back(kv.second);
    }
    for (auto &sp : all) sp->drop_observed();
}

}  // namespace sepfwi
