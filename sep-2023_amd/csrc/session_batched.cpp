// session_batched.cpp -- the batched schedule of a call's shots: every launch advances a whole batch of shots by a
// half step (grids that are not the headline's are launch-bound: the reference issues 24 launches per shot and time step,
// Src/libCUFD.cu:268-332,545-631).  Bf shots share a forward launch, Bb <= Bf a backward launch; per-shot pointers and scalars in a
// device table (ShotDev).
//   batch_ctx / batch_table     a shot in its batch lane; the device table of the call's shots
//   batch_streams               a batch as sub-batches on streams of their own (launches of different queues overlap fill and drain)
//   batched_forward             forward time loop of one batch (+ residuals)
//   batched_backward            backward time loop of one sub-batch
//   run_batched                 the schedule
#include <algorithm>

#include "device_alloc.hpp"
#include "hip_check.hpp"
#include "kernels.hpp"
#include "session.hpp"

namespace sepfwi {

// shot `is` of the call in its batch lane
Session::ShotCtx Session::batch_ctx(const Call &c, int is, int Bf, bool with_obs) {
    return make_ctx(c, is, batch_lane(is % Bf, c.st), with_obs);
}

// the device table of the call's shots (uploaded; the host copy tells the schedule which shots have a fused line of channels)
std::vector<ShotDev> Session::batch_table(const Call &c, int Bf, int Bb) {
    const size_t n = cells_;
    const bool lf = c.opt.line_fuse != 0;
    std::vector<ShotDev> tab(c.group_size);
    gauge_tab_.assign(c.group_size, GaugeShotDev{});
    bool gauged = false;
    for (int is = 0; is < c.group_size; is++) {
        const ShotCtx x = batch_ctx(c, is, Bf, false);
        float *bwd = c.with_adj ? batch_bwd((is % Bf) % Bb) : nullptr;  // backward lane of this shot inside its sub-batch
        ShotDev &d = tab[is] = shot_dev(c, x);
        d.stf = d_stf_.get() + (size_t)is * par_.nSteps;  // the call's source rows, uploaded once (the loop: one row per pass)
        if (bwd) {                                          // a block per batch lane (the loop: the session's own arrays)
            d.bmem = bwd;
            d.adj = bwd_adj(bwd, n);
            d.acc = bwd_acc(bwd, n);
        }
        d.lr_n = lf ? x.line.n : 0;      // a line is fused by the option alone (the loop: not when the shot goes through an injection plan)
        d.nrec = x.gauge ? 0 : x.nrec;  // gauge channels: the generic receiver kernels skip the shot, the gauge twins serve it (side table)
        // read by the forward and the per-step backward kernels only, never by the loop:
        d.mem = state_mem(x.state, n);
        d.syn = x.syn;
        d.comps = x.comps | ((lf && x.line.n > 0 && !(x.comps & 1)) ? 16 : 0);  // bit 16: sample the line inside k_stress
        d.quiet = x.quiet;
        d.rec = x.rec;
        d.sens = x.sens;
        GaugeShotDev &q = gauge_tab_[is];
        if (x.gauge) {
            q.nrec = x.nrec;
            q.comps = x.comps;
            q.rec = x.rec;
            q.tap_start = x.gauge->start.get();
            q.tap_cell = x.gauge->cell.get();
            q.tap_field = x.gauge->field.get();
            q.tap_w = x.gauge->w.get();
            gauged = true;
        }
        if (x.ginj) {
            gauged = true;
            q.nres = x.nres;
            q.ntgt = x.ginj->ntgt;
            q.tgt_start = x.ginj->tgt_start.get();
            q.tgt_cell = x.ginj->tgt_cell.get();
            q.tgt_field = x.ginj->tgt_field.get();
            q.ent_rec = x.ginj->ent_rec.get();
            q.ent_w = x.ginj->ent_w.get();
        }
    }
    HIP_OK(hipMemcpyAsync(d_shots_.get(), tab.data(), tab.size() * sizeof(ShotDev), hipMemcpyHostToDevice, c.st));
    if (gauged) {  // the side table of the gauge twins
        d_gauge_.ensure((size_t)c.group_size);
        HIP_OK(hipMemcpyAsync(d_gauge_.get(), gauge_tab_.data(), gauge_tab_.size() * sizeof(GaugeShotDev), hipMemcpyHostToDevice, c.st));
    }
    if (joint_ && c.with_adj) {  // the backward launches' table: no shot injects a fused line or through the generic receiver kernel
        std::vector<ShotDev> bt = tab;
        for (ShotDev &d : bt) d.lr_n = d.nrec = 0;
        d_shots_bwd_.ensure((size_t)c.group_size);
        HIP_OK(hipMemcpy(d_shots_bwd_.get(), bt.data(), bt.size() * sizeof(ShotDev), hipMemcpyHostToDevice));
    }
    HIP_OK(hipStreamSynchronize(c.st));  // `tab` and `stf_rows` are pageable host memory
    return tab;
}

// The batch `shots` as at most ns sub-batches (schedule.hpp sub_ranges): the first on the call's stream, the others on the extra lanes'
// streams, which start after everything queued on the call's so far
std::vector<Session::SubBatch> Session::batch_streams(hipStream_t st, const std::vector<ShotFacts> &shots, int ns) {
    std::vector<SubBatch> sub;
    for (const SubRange &r : sub_ranges(shots, ns)) {
        if (r.q > 0) ensure_lane_stream(xl_[r.q]);
        sub.push_back(SubBatch{r, r.q > 0 ? xl_[r.q].stream.get() : st});
    }
    if (sub.size() > 1) HIP_OK(hipEventRecord(ev_order_, st));
    for (size_t q = 1; q < sub.size(); q++) HIP_OK(hipStreamWaitEvent(sub[q].st, ev_order_, 0));
    return sub;
}

void Session::batch_join(hipStream_t st, int ns) {  // the call's stream continues when the extra lanes are done
    for (int q = 1; q < ns; q++) {
        HIP_OK(hipEventRecord(xl_[q].join, xl_[q].stream));
        HIP_OK(hipStreamWaitEvent(st, xl_[q].join, 0));
    }
}

// forward time loop of the batch tab[is0 .. is0 + nb), libCUFD.cu:268-332, and its residuals
void Session::batched_forward(Call &c, const std::vector<ShotDev> &tab, int is0, int nb, int split, const std::vector<ShotCtx> &cx) {
    hipStream_t st = c.st;
    const KernelOptions &opt = c.opt;
    const int nSteps = par_.nSteps;
    HIP_OK(hipEventRecord(ev_[0], st));
    for (int k = 0; k < nb; k++) forward_init(cx[k]);
    // the batch as up to three sub-batches on streams of their own (option batch_split).  Per shot: are its channels sampled by the
    // general-receiver launch (not inside k_stress)?  how many gauge channels has it?
    std::vector<ShotFacts> facts((size_t)nb);
    for (int k = 0; k < nb; k++) facts[k] = ShotFacts{!(tab[is0 + k].comps & 16) && tab[is0 + k].nrec > 0, gauge_tab_[is0 + k].nrec};
    const std::vector<SubBatch> sub = batch_streams(st, facts, split);
    for (int it = 0; it <= nSteps - 2; it++)
        for (const SubBatch &b : sub) {
            const ShotDev *shots = d_shots_.get() + is0 + b.a0;
            launch_stress_fwd_batch(b.st, g_, opt, shots, b.n(), md_, pc_, cells_, data_len_, it, c.src_scale, c.with_adj);
            if (c.ph_every > 0 && it % c.ph_every == 0) {  // armed: the sub-batch's shots into the set of its stream (pseudo_hessian.hpp)
                launch_pseudo_hessian_batch(b.st, g_, shots, b.n(), cells_, md_, ph_acc(ph_set_[b.q].get()), (float)c.ph_every);
                cs_.launches++;
            }
            launch_velocity_fwd_batch(b.st, g_, opt, shots, b.n(), md_, pc_, cells_);
            cs_.launches += 2;
            if (b.general) {  // general receivers: ONE launch samples the new state of the sub-batch's shots into column it + 1
                launch_record_batch(b.st, g_, shots, b.n(), survey_.max_nrec, cells_, data_len_, it + 1);
                cs_.launches++;
            }
            if (b.gauge) {  // gauge channels: their twin, from the side table
                launch_record_gauge_batch(b.st, shots, d_gauge_.get() + is0 + b.a0, b.n(), b.gauge, cells_, data_len_, it + 1);
                cs_.launches++;
            }
        }
    batch_join(st, (int)sub.size());
    for (int k = 0; k < nb; k++)
        if (tab[is0 + k].comps & 16) record_column(cx[k], nSteps - 1);
    if (c.if_res && joint_)
        residual_batch(c, cx, nb);
    else if (c.if_res)
        for (int k = 0; k < nb; k++) cond_on_ ? residual_conditioned(c, cx[k]) : residual(cx[k]);
    HIP_OK(hipEventRecord(ev_[1], st));
    cs_.fwd_steps += (long long)nb * (nSteps - 1);
    cs_.fwd_ms += bracket_ms(0, st);
}

// backward time loop of the sub-batch tab[first .. first + nbb) in backward lanes 0 .. nbb-1, libCUFD.cu:500-675
void Session::batched_backward(Call &c, const std::vector<ShotDev> &tab, int first, int nbb, int split, const ShotCtx *cx) {
    hipStream_t st = c.st;
    const Grid &g = g_;
    const KernelOptions &opt = c.opt;
    const int nSteps = par_.nSteps;
    const size_t n = cells_;
    HIP_OK(hipEventRecord(ev_[2], st));
    for (int k = 0; k < nbb; k++) HIP_OK(hipMemsetAsync(batch_bwd(k), 0, kBwdZeroed * n * sizeof(float), st));  // memories + adjoint fields
    for (int k = 0; k < nbb; k++)
        if (cx[k].quiet) HIP_OK(hipMemsetAsync(cx[k].quiet + 2 * (size_t)g.qn, 0, 2 * (size_t)g.qn * sizeof(unsigned int), st));
    // Per shot: is its residual injected by the general-receiver launch (not inside k_bwd_b; a joint misfit: the plan serves every shot)?
    // how many adjoint targets has it as a gauge shot?
    std::vector<ShotFacts> facts((size_t)nbb);
    for (int k = 0; k < nbb; k++) facts[k] = ShotFacts{!joint_ && tab[first + k].lr_n == 0 && tab[first + k].nrec > 0, gauge_tab_[first + k].ntgt};
    const ShotDev *tab_dev = (joint_ ? d_shots_bwd_.get() : d_shots_.get()) + first;
    // An experiment that lost, kept in the -DSEPFWI_PROBES build (option pk_ms; profiles/EXPERIMENTS.md #48): the whole sub-batch as ONE
    // persistent launch (the multi-shot loop, session_persist.cpp) where every shot's channels are a fused line (or absent).  On every
    // grid that takes the batched schedule the per-step launches below are faster, also against the loop without any synchronisation.
    bool lines = opt.pk_ms != 0 && opt.line_fuse != 0 && !joint_;
    for (int k = 0; k < nbb; k++) lines = lines && (tab[first + k].nrec == 0 || tab[first + k].lr_n > 0) && gauge_tab_[first + k].nrec == 0;
    const bool looped = lines && persist_prepare(pk_ms_, opt, nbb) && batched_backward_persistent(c, tab, first, nbb);
    const std::vector<SubBatch> sub = batch_streams(st, facts, looped ? 1 : split);  // sub-batches on streams of their own, as in the forward loop
    for (int it = nSteps - 2; it >= 0 && !looped; it--) {
        const Event *ev = probe_pair(c, it);
        const Grid gs = step_grid(opt, it);
        for (const SubBatch &b : sub) {
            const ShotDev *shots = tab_dev + b.a0;
            launch_bwd_a_batch(b.st, gs, opt, shots, b.n(), md_, pc_, n, it);
            launch_bwd_b_batch(b.st, gs, opt, shots, b.n(), md_, pc_, n, it, c.src_scale, (ev && b.q == 0) ? ev[0].get() : nullptr,
                               (ev && b.q == 0) ? ev[1].get() : nullptr);
            cs_.launches += 2;
            if (b.general) {  // res_injection_exx / _ezz for the sub-batch's shots whose channels are not a fused line: ONE launch
                launch_inject_batch(b.st, g, shots, b.n(), survey_.max_nrec, n, it);
                cs_.launches++;
            }
            if (b.gauge) {  // gauge channels: their twin, from the side table
                launch_inject_gauge_batch(b.st, shots, d_gauge_.get() + first + b.a0, b.n(), b.gauge, n, it);
                cs_.launches++;
            }
        }
    }
    batch_join(st, (int)sub.size());
    HIP_OK(hipEventRecord(ev_[3], st));
    cs_.bwd_steps += (long long)nbb * (nSteps - 1);
    cs_.bwd_ms += bracket_ms(2, st);
    collect_probes(c);
    if (looped) persist_check_pass(pk_ms_);
}

void Session::run_batched(Call &c, const Schedule &s) {
    hipStream_t st = c.st;
    const int nSteps = par_.nSteps, group_size = c.group_size, Bf = s.Bf, Bb = s.Bb;
    const size_t n = cells_;
    ensure_batch(Bf, c.with_adj ? Bb : 0, c.with_adj, group_size);
    HIP_OK(hipMemcpyAsync(d_stf_.get(), c.stf_rows.data(), (size_t)group_size * nSteps * sizeof(float), hipMemcpyHostToDevice, st));
    const std::vector<ShotDev> tab = batch_table(c, Bf, Bb);
    if (c.ph_every > 0) ph_begin(c, s.split);  // one set per sub-batch stream
    if (c.with_adj)
        for (int k = 0; k < Bb; k++) HIP_OK(hipMemsetAsync(bwd_acc(batch_bwd(k), n), 0, kAccArrays * n * sizeof(float), st));
    for (int is0 = 0; is0 < group_size; is0 += Bf) {
        const int nb = std::min(Bf, group_size - is0);
        std::vector<ShotCtx> cx;
        for (int k = 0; k < nb; k++) cx.push_back(batch_ctx(c, is0 + k, Bf, true));
        batched_forward(c, tab, is0, nb, s.split, cx);
        obs_->release_all();
        for (int k = 0; k < nb; k++) after_forward(c, cx[k]);
        for (int kb = 0; c.with_adj && kb < nb; kb += Bb) batched_backward(c, tab, is0 + kb, std::min(Bb, nb - kb), s.split, cx.data() + kb);
    }
    if (c.with_adj)  // the batch lanes' accumulators -> the session's (zeroed in prepare_buffers), summed in lane order
        for (int k = 0; k < Bb; k++) {
            launch_add_inplace(st, acc_.lam, bwd_acc(batch_bwd(k), n), kAccArrays * n);
            cs_.launches++;
        }
}

}  // namespace sepfwi
