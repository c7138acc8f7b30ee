// session_run.cpp -- Session::run, the cufd call (Src/libCUFD.cu:170-724), split into its passes:
//   prepare_media / prepare_buffers     set-up of one call (libCUFD.cu:39-165, the part that is not kept between calls)
//   forward_*  / residual*              forward time loop of one shot and its misfit (libCUFD.cu:268-332, 410-427); the misfit under a
//                                       data-conditioning key, residual_conditioned: session_data.cpp
//   after_forward                       seismogram files / HBM store / scratch dumps (libCUFD.cu:732-769)
//   backward_* / backward               boundary-saving adjoint time loop of one shot (libCUFD.cu:500-675); as one persistent launch:
//                                       session_persist.cpp
//   run_streams                         the stream schedule of a call's shots; the batched one: session_batched.cpp
//   write_outputs                       gradient finalisation and read-back (libCUFD.cu:710-724,775-779)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "das_gauge.hpp"
#include "geophone.hpp"
#include "device_alloc.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "session.hpp"

namespace sepfwi {

static const char *kComp[4] = {"pr", "vx", "vz", "ett"};  // libCUFD.cu:216-223,755-769

static std::string shot_file(const Params &p, int comp, int id) {
    return p.data_dir_name + "/Shot_" + kComp[comp] + std::to_string(id) + ".bin";
}

int ptr_device(const void *p) {  // (session.hpp)
    if (!p) return -1;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // clear: plain host memory is reported as an error on some ROCm versions
        return -1;
    }
    return (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged) ? attr.device : -1;
}

// A NULL stream argument means the legacy default stream, which is what torch's default stream is on ROCm: the call's
// own (non-blocking) stream must not start before the work already queued there -- the Lame maps that produced
// Lambda/Mu/Den, the zero-fill of the gradient tensors -- has finished.
void Session::order_after_null_stream(hipStream_t st) {
    HIP_OK(hipEventRecord(ev_order_, nullptr));
    HIP_OK(hipStreamWaitEvent(st, ev_order_, 0));
}

// ---- set-up of one call ------------------------------------------------------------------------------------------------
// media: boundary arrays -> internal layout, averages, Courant guard (utilities.cu:225-241, libCUFD.cu:90).  Inputs that do
// not live on this session's device (host memory, or another GPU's memory) are staged.
void Session::prepare_media(Call &c, const float *Lambda, const float *Mu, const float *Den) {
    hipStream_t st = c.st;
    const size_t n = cells_, dense = (size_t)par_.nz * (size_t)par_.nx;
    const float *dL = Lambda, *dM = Mu, *dD = Den;
    if (ptr_device(Lambda) != gpu_id_) { HIP_OK(hipMemcpyAsync(in_stage_, Lambda, dense * sizeof(float), hipMemcpyDefault, st)); dL = in_stage_; }
    if (ptr_device(Mu) != gpu_id_) { HIP_OK(hipMemcpyAsync(in_stage_ + dense, Mu, dense * sizeof(float), hipMemcpyDefault, st)); dM = in_stage_ + dense; }
    if (ptr_device(Den) != gpu_id_) { HIP_OK(hipMemcpyAsync(in_stage_ + 2 * dense, Den, dense * sizeof(float), hipMemcpyDefault, st)); dD = in_stage_ + 2 * dense; }
    HIP_OK(hipMemsetAsync(cp2_bits_, 0, sizeof(unsigned int), st));
    float *m[6];  // the arrays of md_, to be written
    for (int k = 0; k < 6; k++) m[k] = media_ + (size_t)k * n;
    launch_model_prep(st, g_, c.opt, dL, dM, dD, m[0], m[1], m[2], m[3], m[4], m[5], cp2_bits_);
    cs_.launches++;
    unsigned int bits = 0;
    HIP_OK(hipMemcpyAsync(&bits, cp2_bits_, sizeof(bits), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    float cp2;
    std::memcpy(&cp2, &bits, sizeof(cp2));
    const float vmax = (float)std::sqrt((double)cp2);
    const float dh_min = (par_.dz < par_.dx) ? par_.dz : par_.dx;
    const float courant = (float)((double)(vmax * par_.dt * sqrtf(2.0f)) * (1.0 / 24.0 + 9.0 / 8.0) / (double)dh_min);
    if (!(courant <= 1.0f)) throw CourantError("Courant number " + std::to_string(courant) + " > 1 (vmax " + std::to_string(vmax) + " m/s)");
}

// boundary-saving storage (Boundary.cu:29-41, allocated on the first gradient call), zeroed accumulators (Model.cu:68-71) and
// misfit, the tapered source traces (row shot_ids[i] of stf, Src_Rec.cu:130-137), the source-gradient rows
void Session::prepare_buffers(Call &c, const float *stf) {
    hipStream_t st = c.st;
    const int nSteps = par_.nSteps;
    const size_t n = cells_;
    if (c.with_adj && !frame_) frame_ = dev<float>(frame_lane_len());
    if (c.with_adj) HIP_OK(hipMemsetAsync(acc_buf_, 0, kAccArrays * n * sizeof(float), st));
    if (c.if_res) HIP_OK(hipMemsetAsync(scal_, 0, 4 * sizeof(double), st));
    if (c.if_res && joint_) HIP_OK(hipMemsetAsync(geo_sums_, 0, 4 * sizeof(double), st));
    c.stf_rows.resize((size_t)c.group_size * nSteps);
    for (int i = 0; i < c.group_size; i++) {
        HIP_OK(hipMemcpy(c.stf_rows.data() + (size_t)i * nSteps, stf + (size_t)c.shot_ids[i] * nSteps, nSteps * sizeof(float), hipMemcpyDefault));
        stf_taper(c.stf_rows.data() + (size_t)i * nSteps, nSteps, par_.dt, 0.001f);
    }
    c.src_scale = (float)std::pow(1500.0, 2);  // utilities.cu:531
    if (c.with_adj) {  // source-time-function gradients of all shots of the call, one row each
        const size_t need = (size_t)c.group_size * nSteps;
        stf_grad_.ensure(need);
        HIP_OK(hipMemsetAsync(stf_grad_.get(), 0, need * sizeof(float), st));
    }
}

// Shot `is` of the call in `lane` (stream_lane, batch_lane).  Acquires the shot's observed gather (held in HBM until the group of
// shots is through: ObservedStore::release_all) unless with_obs is false (geometry only).
Session::ShotCtx Session::make_ctx(const Call &c, int is, const Lane &lane, bool with_obs) {
    const Grid &g = g_;
    ShotCtx x{};
    static_cast<Lane &>(x) = lane;
    x.is = is;
    x.id = c.shot_ids[is];
    x.sh = &survey_.shots[x.id];
    x.nrec = x.sh->nrec;
    x.rec = rec_idx_ + rec_off_[x.id];
    x.sens = (sens_ && !x.sh->sens.empty()) ? sens_ + 3 * (size_t)rec_off_[x.id] : nullptr;
    x.stf_s = c.stf_rows.data() + (size_t)is * par_.nSteps;
    // the observed gathers of the components with a weight; one with weight 0 is never read
    if (c.if_res && with_obs) for_active([&](int comp, int) { x.obs_c[comp] = obs_->acquire(x.id, x.nrec, c.st, comp); });
    x.d_obs = x.obs_c[3];
    x.nres = joint_ ? geo_ncomp_ * x.nrec : x.nrec;
    x.scratch = c.with_adj && !par_.scratch_dir_name.empty();  // libCUFD.cu:732-752
    x.comps = (c.if_res || c.to_store) ? (active_comps() | (x.scratch ? 1 : 0)) : 15;  // (active_comps: 8 unless the misfit is a joint one)
    // horizontal line of consecutive channels inside the computed region?  (channels with a gauge length never are: they are not
    // sampled at their own cells, so the field kernels cannot take them, and quiet_skip stays off for them)
    const Shot &sh = *x.sh;
    const bool gauge = par_.gauge > 1 && x.nrec > 0;
    bool is_line = !gauge && par_.fiber == 0 && !x.sens && x.nrec > 0 && sh.z_rec[0] >= 2 && sh.z_rec[0] <= g.nzc - 3 && sh.x_rec[0] >= 3 && sh.x_rec[0] + x.nrec - 1 <= g.nx - 3;
    for (int r = 1; r < x.nrec && is_line; r++) is_line = (sh.z_rec[r] == sh.z_rec[0] && sh.x_rec[r] == sh.x_rec[0] + r);
    if (is_line) {
        x.line.z = sh.z_rec[0];
        x.line.x0 = sh.x_rec[0];
        x.line.n = x.nrec;
    }
    if (gauge) x.gauge = &gauge_taps(x);
    if ((gauge || (joint_ && x.nrec > 0)) && c.with_adj) x.ginj = &inj_dev(x);  // (a joint misfit: every shot's adjoint source goes through its plan)
    if (!quiet_wanted(c, x)) x.quiet = nullptr;
    x.fld = fields_at(x.state, cells_);
    x.fld.q = x.quiet;
    x.mem = mem_at(state_mem(x.state, cells_), cells_);
    return x;
}

// ---- forward pass of one shot (stream form) ------------------------------------------------------------------------------
// zero the 5 fields + 8 memory variables (libCUFD.cu:175-194); data column 0 stays 0 (:205-209)
void Session::forward_init(const ShotCtx &x) {
    HIP_OK(hipMemsetAsync(x.state, 0, kStateArrays * cells_ * sizeof(float), x.st));
    if (x.quiet) {
        HIP_OK(hipMemsetAsync(x.quiet, 0, 2 * (size_t)g_.qn * sizeof(unsigned int), x.st));  // nothing holds a value yet
        cs_.quiet_last = x.quiet;
    }
    for (int k = 0; k < 4; k++)
        if ((x.comps >> k) & 1) HIP_OK(hipMemsetAsync(syn_of(x, k), 0, (size_t)x.nrec * sizeof(float), x.st));
}

// seismogram column `column` of the shot's present state (recording*, utilities.cu:593-602,645-703)
void Session::record_column(const ShotCtx &x, int column) {
    const size_t col = (size_t)column * x.nrec;
    if (x.gauge)
        launch_record_gauge(x.st, x.fld, x.nrec, x.rec, x.gauge->start.get(), x.gauge->cell.get(), x.gauge->field.get(), x.gauge->w.get(), syn_of(x, 0) + col, syn_of(x, 1) + col,
                            syn_of(x, 2) + col, syn_of(x, 3) + col, x.comps);
    else
        launch_record(x.st, g_, x.fld, x.nrec, x.rec, syn_of(x, 0) + col, syn_of(x, 1) + col, syn_of(x, 2) + col, syn_of(x, 3) + col, x.comps, x.sens);
    cs_.launches++;
}

// taps of a shot's gauge channels (das_gauge.hpp), uploaded once per session and shot
const Session::GaugeDev &Session::gauge_taps(const ShotCtx &x) {
    auto it = gauge_.find(x.id);
    if (it != gauge_.end()) return it->second;
    const Shot &sh = *x.sh;
    const GaugeTaps t = make_gauge_taps(sh.nrec, sh.z_rec.data(), sh.x_rec.data(), sh.sens.empty() ? nullptr : sh.sens.data(), par_.fiber != 0,
                                        g_.dx * g_.rdz, par_.gauge);
    std::vector<int> cell(t.w.size());
    for (size_t e = 0; e < cell.size(); e++) cell[e] = t.z[e] * g_.pitch + t.x[e];
    GaugeDev d;
    d.start = upload(t.start);
    d.cell = upload(cell);
    d.field = upload(t.field);
    d.w = upload(t.w);
    return gauge_.emplace(x.id, std::move(d)).first->second;
}

// one forward time step (libCUFD.cu:268-332); inl: the line of channels is sampled inside k_stress
void Session::forward_step(const Call &c, const ShotCtx &x, int it, bool inl) {
    float *frame_t = c.with_adj ? x.frame + (size_t)it * 5 * (size_t)g_.frame_len : nullptr;
    const float amp = c.src_scale * x.stf_s[it] * par_.dt;
    LineRec lr{};
    if (inl && it >= 1) {
        lr = x.line;
        const size_t c0 = (size_t)it * x.nrec;
        lr.d_vx = (x.comps & 2) ? syn_of(x, 1) + c0 : nullptr;
        lr.d_vz = (x.comps & 4) ? syn_of(x, 2) + c0 : nullptr;
        lr.d_ett = (x.comps & 8) ? syn_of(x, 3) + c0 : nullptr;
    }
    launch_stress_fwd(x.st, g_, c.opt, x.fld, x.mem, md_, pc_, frame_t, x.sh->z_src, x.sh->x_src, amp, lr);
    if (x.ph && it % c.ph_every == 0) {  // armed: velocities of the start of the step, stresses after update and source add (pseudo_hessian.hpp)
        launch_pseudo_hessian(x.st, g_, x.fld, md_, ph_acc(x.ph), (float)c.ph_every);
        cs_.launches++;
    }
    launch_velocity_fwd(x.st, g_, c.opt, x.fld, x.mem, md_, pc_);
    cs_.launches += 2;
    if (!inl) record_column(x, it + 1);
}

// residual + misfit of the axial-strain component (libCUFD.cu:413,418,427)
void Session::residual(const ShotCtx &x) {
    if (joint_) {  // geophone.hip: the weighted residuals of the active components as one array [it][C nrec], sum r_c^2 per component
        launch_geo_residual(x.st, geo_res_shot(x), par_.nSteps, geo_sums_);
        cs_.launches++;
        return;
    }
    launch_residual(x.st, x.d_obs, syn_of(x, 3), x.res, x.nrec, (long long)x.nrec * par_.nSteps, scal_);
    cs_.launches++;
}

GeoResShot Session::geo_res_shot(const ShotCtx &x) const {
    GeoResShot q{};
    q.res = x.res;
    q.nrec = x.nrec;
    q.nblk = geo_ncomp_;
    for_active([&](int comp, int b) {
        q.obs[b] = x.obs_c[comp];
        q.syn[b] = syn_of(x, comp);
        q.w[b] = par_.weight(comp);
        q.slot[b] = comp - 1;
    });
    return q;
}

// the joint residual of the batch's shots in ONE launch (the table is uploaded from a member: it outlives the copy)
void Session::residual_batch(const Call &c, const std::vector<ShotCtx> &cx, int nb) {
    geo_res_tab_.assign((size_t)nb, GeoResShot{});
    int max_nrec = 0;
    for (int k = 0; k < nb; k++) {
        geo_res_tab_[k] = geo_res_shot(cx[k]);
        max_nrec = std::max(max_nrec, cx[k].nrec);
    }
    d_geo_res_.ensure((size_t)nb);
    HIP_OK(hipMemcpyAsync(d_geo_res_.get(), geo_res_tab_.data(), (size_t)nb * sizeof(GeoResShot), hipMemcpyHostToDevice, c.st));
    launch_geo_residual_batch(c.st, d_geo_res_.get(), nb, max_nrec, geo_ncomp_, par_.nSteps, geo_sums_);
    cs_.launches++;
}

// ---- what a forward pass leaves behind -----------------------------------------------------------------------------------
// observe: export the four gathers as [nrec][nSteps] files (libCUFD.cu:755-769)
void Session::export_gathers(const Call &c, const ShotCtx &x) {
    hipStream_t st = c.st;
    const size_t cnt = (size_t)x.nrec * par_.nSteps;
    for (int k = 0; k < 4; k++) {
        launch_transpose(st, syn_of(x, k), xpose_, par_.nSteps, x.nrec);  // [it][rec] -> [rec][it]
        HIP_OK(hipMemcpyAsync(h_io_.get(), xpose_, cnt * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        const std::string fn = shot_file(par_, k, x.id);
        FILE *fp = fopen(fn.c_str(), "wb");
        if (!fp) throw IoError("cannot write '" + fn + "'");  // utilities.cu:22-31
        const size_t w = fwrite(h_io_.get(), sizeof(float), cnt, fp);
        fclose(fp);
        if (w != cnt) throw IoError("short write on '" + fn + "'");
    }
    obs_->forget(x.id);  // a cached gather of this shot is stale: the file just changed
}

// optional scratch dumps of the PRESSURE component, [nrec][nSteps] float32 (libCUFD.cu:732-745): Syn_Shot{id}.bin,
// CondObs_Shot{id}.bin (observed data, unconditioned here as there) and Residual_Shot{id}.bin = obs - syn with the first time
// sample zeroed (gpuMinus, utilities.cu:154-167)
void Session::scratch_dumps(const Call &c, const ShotCtx &x) {
    hipStream_t st = c.st;
    const int nSteps = par_.nSteps;
    const size_t cnt = (size_t)x.nrec * nSteps;
    launch_transpose(st, syn_of(x, 0), xpose_, nSteps, x.nrec);
    HIP_OK(hipMemcpyAsync(h_io_.get(), xpose_, cnt * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    std::vector<float> obs_pr(cnt);
    {
        const std::string fn = shot_file(par_, 0, x.id);
        FILE *fp = fopen(fn.c_str(), "rb");
        if (!fp) throw IoError("cannot read observed data '" + fn + "'");
        const size_t got = fread(obs_pr.data(), sizeof(float), cnt, fp);
        fclose(fp);
        if (got != cnt) throw IoError("short read on '" + fn + "'");
    }
    auto dump = [&](const char *stem, const float *data) {
        const std::string fn = par_.scratch_dir_name + "/" + stem + std::to_string(x.id) + ".bin";
        FILE *fp = fopen(fn.c_str(), "wb");
        if (!fp) throw IoError("cannot write '" + fn + "'");
        const size_t w = fwrite(data, sizeof(float), cnt, fp);
        fclose(fp);
        if (w != cnt) throw IoError("short write on '" + fn + "'");
    };
    dump("Syn_Shot", h_io_.get());
    dump("CondObs_Shot", obs_pr.data());
    for (int r = 0; r < x.nrec; r++) {
        float *o = obs_pr.data() + (size_t)r * nSteps;
        const float *sy = h_io_.get() + (size_t)r * nSteps;
        o[0] = 0.0f;
        for (int t = 1; t < nSteps; t++) o[t] = o[t] - sy[t];
    }
    dump("Residual_Shot", obs_pr.data());
}

void Session::after_forward(Call &c, const ShotCtx &x) {
    if (c.to_store) {  // calc_id 3: the modelled gathers of the components with a weight (by default the axial strain alone) become the
        // shot's observed data, exactly as sepfwi_set_observed would install the files of calc_id 2
        for_active([&](int comp, int) { obs_->put_device_gather(x.id, syn_of(x, comp), x.nrec, c.st, comp); });
    } else if (!c.if_res)
        export_gathers(c, x);
    else if (x.scratch)
        scratch_dumps(c, x);
}

// ---- backward pass of one shot (stream form) -----------------------------------------------------------------------------
// adjoint fields + all eight memory variables restart from zero (:503-515); the two pre-loop adjoint launches (:520-542) act on
// all-zero arrays and change nothing.
void Session::backward_init(const BwdLane &L) {
    HIP_OK(hipMemsetAsync(L.bm.dvz_dz, 0, kMemArrays * cells_ * sizeof(float), L.s));
    HIP_OK(hipMemsetAsync(L.adj.vz, 0, kFieldArrays * cells_ * sizeof(float), L.s));
}

// HIP-event pair for this step's k_bwd_b launch (option probe: every probe-th step), or null
const Event *Session::probe_pair(Call &c, int it) {
    if (c.opt.probe <= 0 || c.n_probe >= kProbePairs || (it % c.opt.probe) != 0) return nullptr;
    return &probe_ev_[2 * c.n_probe++];
}

void Session::collect_probes(Call &c) {  // after a synchronisation of the main stream
    for (int k = 0; k < c.n_probe; k++) {
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, probe_ev_[2 * k], probe_ev_[2 * k + 1]));
        cs_.probe_us += 1e3 * ms;
        cs_.probe_calls++;
    }
    c.n_probe = 0;
}

Grid Session::step_grid(const KernelOptions &opt, int it) const {
    Grid gs = g_;
    if (opt.img_every > 1) gs.dt_img = (it % opt.img_every == 0) ? (float)opt.img_every * g_.dt : 0.0f;
    return gs;
}

// one backward time step, the reference's order (libCUFD.cu:545-631)
void Session::backward_step(Call &c, const ShotCtx &x, const BwdLane &L, int it) {
    const Grid &g = g_;
    const KernelOptions &opt = c.opt;
    const bool inj_inl = inject_inline(c, x);
    const Shot &sh = *x.sh;
    float *frame_t = x.frame + (size_t)it * 5 * (size_t)g.frame_len;
    float *sg = stf_grad_.get() + (size_t)x.is * par_.nSteps + it;
    const float amp = c.src_scale * x.stf_s[it] * par_.dt;
    const float *res_t = x.res + (size_t)it * x.nres;
    LineRec lr{};
    if (inj_inl) {
        lr = x.line;
        lr.res = res_t;
    }
    const Grid gs = step_grid(opt, it);
    if (opt.bwd_fuse != 0) {
        const Event *ev = probe_pair(c, it);
        Fields adj = L.adj;  // (the adjoint maps follow the shot's lane; the residual enters inside k_bwd_b, which marks the channels' segments)
        adj.q = x.quiet ? x.quiet + 2 * (size_t)g.qn : nullptr;
        launch_bwd_a(L.s, gs, opt, x.fld, L.bm, md_, pc_, frame_t, adj, L.acc);
        launch_bwd_b(L.s, gs, opt, x.fld, L.bm, md_, pc_, frame_t, sh.z_src, sh.x_src, amp, (float)sh.src_rxz, sg, adj, L.acc, lr, ev ? ev[0].get() : nullptr,
                     ev ? ev[1].get() : nullptr);
        if (!inj_inl) inject_column(x, L, res_t);
        cs_.launches += inj_inl ? 2 : 3;
    } else {  // the reference's launch structure
        launch_velocity_rev(L.s, gs, opt, x.fld, md_, pc_, frame_t, sh.z_src, sh.x_src, (float)sh.src_rxz, sg, L.adj, L.acc);
        launch_stress_rev(L.s, gs, opt, x.fld, md_, pc_, frame_t, sh.z_src, sh.x_src, amp, L.adj, L.acc);
        launch_velocity_adj(L.s, g, opt, L.adj, L.bm, md_, pc_);
        inject_column(x, L, res_t);
        launch_stress_adj(L.s, g, opt, L.adj, L.bm, md_, pc_);
        cs_.launches += 5;
    }
}

// this step's adjoint source: res_injection_exx / _ezz per channel (k_inject), or a gauge shot's plan, one add per target (k_inject_gauge)
void Session::inject_column(const ShotCtx &x, const BwdLane &L, const float *res_t) {
    if (x.ginj)
        launch_inject_gauge(L.s, L.adj, x.ginj->ntgt, res_t, x.ginj->tgt_start.get(), x.ginj->tgt_cell.get(), x.ginj->tgt_field.get(), x.ginj->ent_rec.get(),
                            x.ginj->ent_w.get());
    else
        launch_inject(L.s, g_, L.adj, x.nrec, x.rec, res_t, x.sens);
}

// The backward pass of one shot: ONE persistent launch where the configuration allows it (session_persist.cpp), else -- or when the
// loop's start rendezvous says the grid is not resident at once, which leaves everything untouched -- one backward_step per time step.
void Session::backward(Call &c, const ShotCtx &x) {
    hipStream_t st = c.st;
    const BwdLane L{st, mem_, adj_, acc_};
    const bool eligible = persist_ready(c, x);
    HIP_OK(hipEventRecord(ev_[2], st));
    backward_init(L);
    if (x.quiet) HIP_OK(hipMemsetAsync(x.quiet + 2 * (size_t)g_.qn, 0, 2 * (size_t)g_.qn * sizeof(unsigned int), st));  // the adjoint maps
    const bool looped = eligible && backward_persistent(c, x, L);
    if (!looped)
        for (int it = par_.nSteps - 2; it >= 0; it--) backward_step(c, x, L, it);
    HIP_OK(hipEventRecord(ev_[3], st));
    cs_.bwd_steps += (long long)(par_.nSteps - 1);
    cs_.bwd_ms += bracket_ms(2, st);
    collect_probes(c);
    if (looped) persist_check_pass(pk_);
}

// ---- stream schedule: up to fwd_lanes forward passes side by side (their kernel-boundary gaps and tails fill each other:
// x1.28 on the forward loops with three lanes), then their backward passes one after the other (two of them together lose
// 13-20 %)
void Session::run_streams(Call &c, int n_lanes) {
    hipStream_t st = c.st;
    const int nSteps = par_.nSteps;
    if (n_lanes >= 2) ensure_lanes(n_lanes, c.with_adj);
    if (c.ph_every > 0) ph_begin(c, n_lanes);  // (before ev_[0]: the extra lanes start after the sets are zeroed)
    for (int is = 0; is < c.group_size;) {
        const int np = std::min(n_lanes, c.group_size - is);
        ShotCtx ctx[kMaxLanes];
        for (int k = 0; k < np; k++) {
            ctx[k] = make_ctx(c, is + k, stream_lane(k, st));
            if (c.ph_every > 0) ctx[k].ph = ph_set_[k].get();  // armed: the accumulator set of the lane
        }

        // forward time loop(s), libCUFD.cu:268-332
        HIP_OK(hipEventRecord(ev_[0], st));
        for (int k = 1; k < np; k++) HIP_OK(hipStreamWaitEvent(xl_[k].stream, ev_[0], 0));  // extra lanes start after everything queued so far
        for (int k = 0; k < np; k++) forward_init(ctx[k]);
        bool inl[kMaxLanes];
        for (int k = 0; k < np; k++) inl[k] = forward_inline(c, ctx[k]);
        for (int it = 0; it <= nSteps - 2; it++)
            for (int k = 0; k < np; k++) forward_step(c, ctx[k], it, inl[k]);
        for (int k = 0; k < np; k++)
            if (inl[k]) record_column(ctx[k], nSteps - 1);
        if (c.if_res && !cond_on_)
            for (int k = 0; k < np; k++) residual(ctx[k]);
        batch_join(st, np);
        if (c.if_res && cond_on_)
            for (int k = 0; k < np; k++) residual_conditioned(c, ctx[k]);
        HIP_OK(hipEventRecord(ev_[1], st));
        cs_.fwd_steps += (long long)np * (nSteps - 1);
        cs_.fwd_ms += bracket_ms(0, st);
        obs_->release_all();  // the residuals are formed: the group's observed gathers may leave HBM again

        for (int k = 0; k < np; k++) after_forward(c, ctx[k]);
        if (c.with_adj)
            for (int k = 0; k < np; k++) backward(c, ctx[k]);
        is += np;
    }
}

// ---- diagonal pseudo-Hessian (pseudo_hessian.hpp) ---------------------------------------------------------------------------
// The accumulator sets of an armed call, one per forward lane (stream schedule) or sub-batch stream (batched schedule): allocated on
// first use, zeroed on the call's stream at the start of every armed call -- the result is that call's own.
void Session::ph_begin(Call &c, int nsets) {
    nsets = std::max(1, std::min(nsets, (int)kPhMaxSets));
    for (int k = 0; k < nsets; k++) {
        if (!ph_set_[k]) ph_set_[k] = dev<float>(3 * cells_);
        HIP_OK(hipMemsetAsync(ph_set_[k].get(), 0, 3 * cells_ * sizeof(float), c.st));
    }
    ph_nsets_ = nsets;
}

void Session::pseudo_hessian_arm(int every) {
    std::lock_guard<std::mutex> lock(mu_);
    if (every < 0) throw std::invalid_argument("pseudo-Hessian: every must be >= 0");
    if (every > 0 && par_.nPml < 2) throw std::invalid_argument("pseudo-Hessian: needs nPml >= 2 (the stencils of the interior reach two cells out)");
    if (every > 0 && !ph_out_) {  // first arming: the result arrays and the first accumulator set
        HIP_OK(hipSetDevice(gpu_id_));
        ph_out_ = dev<float>(3 * (size_t)par_.nz * (size_t)par_.nx);
        if (!ph_set_[0]) ph_set_[0] = dev<float>(3 * cells_);
    }
    ph_every_ = every;
}

void Session::pseudo_hessian_get(float *hLambda, float *hMu, float *hDen) {
    std::lock_guard<std::mutex> lock(mu_);
    if (!ph_valid_) throw std::invalid_argument("pseudo-Hessian: no armed call yet");
    HIP_OK(hipSetDevice(gpu_id_));
    HIP_OK(hipDeviceSynchronize());  // (a call on a caller's stream with async set may still be running)
    const size_t dense = (size_t)par_.nz * (size_t)par_.nx;
    float *out[3] = {hLambda, hMu, hDen};
    for (int k = 0; k < 3; k++)
        if (out[k]) HIP_OK(hipMemcpy(out[k], ph_out_.get() + (size_t)k * dense, dense * sizeof(float), hipMemcpyDefault));
}

// ---- outputs: written in place when they live on this device, staged otherwise (host memory, another GPU) ------------------
void Session::write_outputs(Call &c, float *misfit, float *grad_Lambda, float *grad_Mu, float *grad_Den, float *grad_stf) {
    hipStream_t st = c.st;
    const size_t dense = (size_t)par_.nz * (size_t)par_.nx;
    if (c.with_adj && grad_stf) {  // rows indexed by local shot position (libCUFD.cu:671-673)
        std::vector<float> h_gstf((size_t)c.group_size * par_.nSteps);
        HIP_OK(hipMemcpy(h_gstf.data(), stf_grad_.get(), h_gstf.size() * sizeof(float), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(grad_stf, h_gstf.data(), h_gstf.size() * sizeof(float), hipMemcpyDefault));
    }
    if (c.with_adj) {
        const GradOut o = grad_out(grad_Lambda, grad_Mu, grad_Den);
        launch_finalize_gradients(st, g_, md_, acc_, o.dev[0], o.dev[1], o.dev[2]);
        cs_.launches++;
        copy_staged(o, st);
    }
    if (c.ph_every > 0) {  // the sets summed in lane order, the constants of pseudo_hessian.hpp
        PhSets sets{};
        sets.nsets = ph_nsets_;
        for (int k = 0; k < ph_nsets_; k++) sets.set[k] = ph_set_[k].get();
        const double mdt = 1e6 * (double)g_.dt;
        launch_pseudo_hessian_finalize(st, g_, sets, cells_, 2.0 * mdt * mdt, mdt * mdt, (double)g_.dt * (double)g_.dt, ph_out_.get(), ph_out_.get() + dense,
                                       ph_out_.get() + 2 * dense);
        cs_.launches++;
        ph_valid_ = true;
    }
    if (c.if_res && misfit) read_misfit(c, misfit, true);
}

Session::GradOut Session::grad_out(float *gLambda, float *gMu, float *gDen) const {
    const size_t dense = (size_t)par_.nz * (size_t)par_.nx;
    GradOut o{{gLambda, gMu, gDen}, {}};
    for (int k = 0; k < 3; k++) o.dev[k] = ptr_device(o.out[k]) == gpu_id_ ? o.out[k] : grad_stage_ + (size_t)k * dense;
    return o;
}

void Session::copy_staged(const GradOut &o, hipStream_t st) {
    const size_t dense = (size_t)par_.nz * (size_t)par_.nx;
    for (int k = 0; k < 3; k++)
        if (o.dev[k] != o.out[k]) HIP_OK(hipMemcpyAsync(o.out[k], o.dev[k], dense * sizeof(float), hipMemcpyDefault, st));
}

void Session::read_misfit(const Call &c, float *misfit, bool parts) {
    hipStream_t st = c.st;
    double sumsq = 0.0, s[3] = {0.0, 0.0, 0.0};  // sum r_c^2 per component (vx, vz, ett)
    HIP_OK(hipMemcpyAsync(&sumsq, scal_, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    s[2] = sumsq;
    if (joint_) {  // -> the weighted misfit and the unweighted parts
        HIP_OK(hipMemcpyAsync(s, geo_sums_, sizeof(s), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        sumsq = 0.0;
        for (int comp = 1; comp <= 3; comp++) sumsq += (double)par_.weight(comp) * s[comp - 1];
    }
    if (parts)
        for (int k = 0; k < 3; k++) parts_[k] = 0.5 * s[k];
    const float mf = (float)(0.5 * sumsq);  // libCUFD.cu:776
    HIP_OK(hipMemcpy(misfit, &mf, sizeof(float), hipMemcpyDefault));
}

// ---- how every call opens and closes (run below, born: session_born.cpp, adjoint_exact: session_exact.cpp) ----------------------
void Session::check_shot_ids(int group_size, const int *shot_ids) const {
    for (int i = 0; i < group_size; i++) {
        const int id = shot_ids[i];
        if (id < 0 || id >= (int)survey_.shots.size() || !survey_.shots[id].present)
            throw std::invalid_argument("shot id " + std::to_string(id) + " is not in the survey file");
    }
}

Session::Call Session::begin_call(hipStream_t ext_stream, int group_size, const int *shot_ids) {
    Call c;
    c.t_begin = std::chrono::steady_clock::now();
    HIP_OK(hipSetDevice(gpu_id_));
    c.opt = kernel_options();  // ONE snapshot for the whole call
    c.st = ext_stream ? ext_stream : own_stream_.get();
    if (!ext_stream) order_after_null_stream(c.st);
    c.group_size = group_size;
    c.shot_ids = shot_ids;
    cs_ = CallStats{};
    check_shot_ids(group_size, shot_ids);
    return c;
}

// HBM budget of the observed-data store: parameter key "obs_cache_mb", else the option of the same name (0: unlimited)
void Session::obs_begin(const Call &c) {
    const long long mb = par_.obs_cache_mb > 0 ? par_.obs_cache_mb : c.opt.obs_cache_mb;
    obs_->set_budget_bytes(mb * 1000000LL);
    obs_->release_all();
}

void Session::end_call(const Call &c, bool sync) {
    if (sync) HIP_OK(hipStreamSynchronize(c.st));
    total_ms_ = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c.t_begin).count();
    last_shots_ = c.group_size;
}

double Session::bracket_ms(int a, hipStream_t st) {
    HIP_OK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, ev_[a], ev_[a + 1]));
    return ms;
}

// ---- the cufd call -------------------------------------------------------------------------------------------------------
void Session::run(float *misfit, float *grad_Lambda, float *grad_Mu, float *grad_Den, float *grad_stf, const float *Lambda, const float *Mu,
                  const float *Den, const float *stf, int calc_id, int group_size, const int *shot_ids, hipStream_t ext_stream, bool async) {
    std::lock_guard<std::mutex> lock(mu_);
    Call c = begin_call(ext_stream, group_size, shot_ids);
    c.if_res = (calc_id == 0 || calc_id == 1);  // Parameter.cpp:125-137
    c.with_adj = (calc_id == 1);
    c.to_store = (calc_id == SEPFWI_CALC_OBSERVE_TO_STORE);  // observe, but into the HBM store instead of the four files
    c.ph_every = c.if_res ? ph_every_ : 0;  // calc_id 2 and 3 never accumulate
    obs_begin(c);

    prepare_media(c, Lambda, Mu, Den);
    prepare_buffers(c, stf);
    // (per shot: one gather per component with a weight)
    const size_t gather_bytes = (size_t)std::max(1, survey_.max_nrec) * par_.nSteps * sizeof(float) * (size_t)geo_ncomp_;
    if (c.if_res && obs_->budget_bytes() == 0)  // observed data of every shot of the call resident before the time loops start
        for (int is = 0; is < group_size; is++)
            for_active([&](int comp, int) { (void)obs_->acquire(shot_ids[is], survey_.shots[shot_ids[is]].nrec, c.st, comp); });
    obs_->release_all();

    // The schedule (schedule.hpp plan_schedule; tests/native/schedule_check.cpp pins the grids named here).  Backward passes that fit
    // the budget together: 2000x500: 2 (and 7 forward); a 101x201 notebook problem: all its shots at once.  Where fewer than three fit
    // the stream schedule runs them one by one -- as the persistent loop where it is eligible: measured fwd+adj at 1000 steps, batched /
    // streams in Gcell-updates/s: 2000x500 (2 fit) 73.5 / 79.6, 1500x500 (3) 77.1 / 75.0, 1000x700 (3) 73.2 / 72.5, 2000x300 (3) 73.7 /
    // 66.1, 1000x500 (5) 69.0 / 63.9 (profiles/r05_other_grids.txt).
    ScheduleIn in;
    in.array_bytes = cells_ * sizeof(float);
    in.batch = c.opt.batch;
    in.batch_f = c.opt.batch_f;
    in.batch_b = c.opt.batch_b;
    in.batch_mb = c.opt.batch_mb;
    in.bwd_fuse = c.opt.bwd_fuse;
    in.pair_fwd = c.opt.pair_fwd;
    in.fwd_lanes = c.opt.fwd_lanes;
    in.batch_split = c.opt.batch_split;
    in.group_size = group_size;
    in.with_adj = c.with_adj;
    in.if_res = c.if_res;
    const Schedule s = plan_schedule(in, [&](int want) { return obs_->max_group(gather_bytes, want); });
    last_batched_ = s.batched;
    if (s.batched)
        run_batched(c, s);
    else
        run_streams(c, s.lanes);
    write_outputs(c, misfit, grad_Lambda, grad_Mu, grad_Den, grad_stf);
    if (!async) {
        HIP_OK(hipStreamSynchronize(c.st));
    } else if (!ext_stream) {  // later work on the default stream sees this call's outputs
        HIP_OK(hipEventRecord(ev_order_, c.st));
        HIP_OK(hipStreamWaitEvent(nullptr, ev_order_, 0));
    }
    if (cs_.quiet_last) {  // how much of the grid the last shot's forward field reached (sepfwi_stats)
        std::vector<unsigned int> bits((size_t)g_.qn);
        HIP_OK(hipMemcpyAsync(bits.data(), cs_.quiet_last + g_.qn, bits.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, c.st));
        HIP_OK(hipStreamSynchronize(c.st));
        for (unsigned int w : bits) cs_.quiet_active += __builtin_popcount(w);
        cs_.quiet_total = (long long)(g_.nzc - 4) * ((g_.nx + 63) / 64);
    }
    end_call(c, false);  // (synchronised above, or left running: async)
    last_calc_ = calc_id;
}

}  // namespace sepfwi
