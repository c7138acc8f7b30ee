// session.hpp -- persistent propagation session (see session.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sepfwi.h"
#include "conditioning.hpp"
#include "config.hpp"
#include "device_alloc.hpp"
#include "errors.hpp"
#include "fwi_types.hpp"
#include "kernels.hpp"
#include "obs_store.hpp"
#include "persist_plan.hpp"
#include "pseudo_hessian.hpp"
#include "schedule.hpp"

namespace sepfwi {

// Device that owns `p`, or -1 for host memory.  A pointer on ANOTHER device than the session's (the single-process
// ngpu > 1 path handing GPU-0 tensors to the session of GPU i) is staged like host memory: the kernels only ever touch
// memory of their own device, peer access is never assumed.
int ptr_device(const void *p);

class Session {
  public:
    Session(const std::string &para_fname, int gpu_id, const std::string &para_text, const std::string &survey_text,
            const Params &par, const Survey &survey);
    ~Session();
    Session(const Session &) = delete;
    Session &operator=(const Session &) = delete;

    bool matches(const std::string &ptext, const std::string &stext) const { return ptext == para_text_ && stext == survey_text_; }
    void run(float *misfit, float *grad_Lambda, float *grad_Mu, float *grad_Den, float *grad_stf, const float *Lambda,
             const float *Mu, const float *Den, const float *stf, int calc_id, int group_size, const int *shot_ids,
             hipStream_t ext_stream, bool async);
    void stats(sepfwi_stats *out) const;
    std::string loop_status();  // "" while the persistent backward loop is in use, else why not (sepfwi_loop_status)
    void drop_observed();
    // observed axial strain of one shot from memory ([nrec][nSteps] like the files; host or device pointer)
    void set_observed(int shot_id, const float *ett, int nrec, int nSteps, int comp = 3);  // comp: 1 vx, 2 vz, 3 ett
    // unweighted 0.5 sum_shots sum r_c^2 of the last misfit or gradient call for (vx, vz, ett); 0 for a component with weight 0
    void misfit_parts(double parts[3]);
    // diagonal pseudo-Hessian (pseudo_hessian.hpp): every >= 1 arms the misfit / gradient calls that follow, 0 disarms; the result of
    // the most recent armed call, dense (nz, nx) each, host or device pointers, any of them null
    void pseudo_hessian_arm(int every);
    void pseudo_hessian_get(float *hLambda, float *hMu, float *hDen);
    // Born modelling and the Gauss-Newton product (session_born.cpp, sepfwi_born): the scattered gathers of v = (dLambda, dMu, dDen),
    // shot after shot as [nrec][nSteps], each output optional; hv_* all null (J v only) or all set (J^T W J v, summed over the shots)
    // dStf (sepfwi_born_src; (group_size, nSteps), row i the call's shot i, host or device): the scattered field's own source term, J [v; ds];
    // v may then be absent (all three null).  hv_stf (exact only): the source block of the product, the layout of dStf
    void born(float *d_ett, float *d_vx, float *d_vz, float *hv_Lambda, float *hv_Mu, float *hv_Den, const float *Lambda, const float *Mu,
              const float *Den, const float *dLambda, const float *dMu, const float *dDen, const float *stf, int group_size, const int *shot_ids,
              hipStream_t ext_stream, bool exact = false, const float *dStf = nullptr, float *hv_stf = nullptr);
    // The exact discrete adjoint (exact_adjoint.hpp, session_exact.cpp, sepfwi_adjoint_exact): g = J^T w for the caller's w (any of
    // w_ett, w_vx, w_vz set; gathers as born() writes them), or, with all of them null, the exact gradient on Omega of the session's
    // misfit and the misfit itself.  (The product P J^T W J P v is born(..., exact = true).)
    void adjoint_exact(float *misfit, float *g_Lambda, float *g_Mu, float *g_Den, const float *w_ett, const float *w_vx, const float *w_vz,
                       const float *Lambda, const float *Mu, const float *Den, const float *stf, int group_size, const int *shot_ids,
                       hipStream_t ext_stream, float *g_stf = nullptr);  // g_stf: the source block J_s^T (.), (group_size, nSteps), or null
    // The conditioning operator of the parameter file (sepfwi_condition): C, or C^T, in place on gathers laid out like born()'s d_ett,
    // host or device; the identity when no conditioning key is live
    void condition(float *data, bool transpose, int group_size, const int *shot_ids, hipStream_t ext_stream);
    // The misfit of the parameter file in data space (sepfwi_data_misfit, sepfwi_data_gn; session_data.cpp): raw gathers laid out like
    // born()'s d_ett, host or device.  Neither the observed store nor the misfit, misfit parts or statistics of the last call are touched.
    void data_misfit(float *misfit, float *adj, const float *obs, const float *syn, int group_size, const int *shot_ids, hipStream_t ext_stream);
    // obs: the observed gathers (sepfwi_data_gn_obs: obs_entry), needed under robust_misfit alone and not read otherwise; may be null then
    void data_gn(float *out, const float *obs, const float *syn, const float *d, int group_size, const int *shot_ids, hipStream_t ext_stream, bool obs_entry);
    // test hook: wavefield `which` (0..4 vz, vx, szz, sxx, sxz; 5..9 their adjoint twins) of forward lane `lane` as left
    // by the last call, dense (nz - nPad, nx) row-major, host or device pointer; 10..14: the scattered fields of the last Born call
    void copy_field(int lane, int which, float *out);
    const Params &params() const { return par_; }

  private:
    template <class T> T *dalloc(size_t n);
    void init_grid();        // constructor steps
    void alloc_arrays();
    void upload_profiles();
    void upload_survey();
    void ensure_lanes(int n_lanes, bool with_frames);
    void ensure_batch(int n_fwd, int n_bwd, bool with_frames, int n_shots);
    void order_after_null_stream(hipStream_t st);
    // ---- the data-conditioning chain (session_data.cpp), on [rec][it] gathers of one shot ---------------------------------------
    // C of the parameter file on one gather in place: window (if_win: per channel, with weights; else the end taper), then band-pass
    // (filter), then the fan filter across the channels (fk_slowness); and C^T: fan filter, band-pass, then window
    void window_gather(hipStream_t st, float *gather, int shot_id, int nrec);
    void condition_gather(hipStream_t st, float *gather, int shot_id, int nrec);
    void condition_gather_t(hipStream_t st, float *gather, int shot_id, int nrec);
    // What a call runs between its two transpositions, and the data-space entry points on a caller's gathers.
    //   misfit_chain  obs_c: the shot's CONDITIONED observed gather, only read.  syn: the raw synthetic gather, conditioned (under
    //                 if_src_update also updated) in place.  out: the raw-space adjoint source.  The misfit's sum is added to *acc.
    //   gn_chain      d: the raw gather, conditioned in place.  bg: the raw background gather, conditioned in place, under
    //                 if_envelope_misfit and robust_misfit; else null.  obs_c: C obs, read under robust_misfit alone.  out = sign C^T Z C d,
    //                 sign C^T D^T Z D C d, or sign C^T Z W Z C d with the IRLS weight W of (obs_c, C bg).
    //                 The misfit kind is the file's: L2, if_cross_misfit, if_envelope_misfit, if_w2_misfit or robust_misfit.
    // ALIASING: the gathers of one call are all different (the envelope and W2 kernels read the other two while they write out).  The callers
    // pass the session's scratch gathers xpose_, xpose2_, xpose3_.
    void misfit_chain(hipStream_t st, const float *obs_c, float *syn, float *out, int shot_id, int nrec, double *acc);
    void gn_chain(hipStream_t st, float *d, float *bg, float *out, int shot_id, int nrec, float sign, const float *obs_c = nullptr);
    void ensure_data_scratch();  // xpose3_ / data_acc_
    // prologue and shot loop of condition / data_misfit / data_gn: this device and the caller's stream, or the session's own ordered after
    // the null stream; f(shot id, nrec, offset in the caller's arrays, length) for every shot with channels
    hipStream_t data_stream(hipStream_t ext_stream);
    template <class F> void for_each_gather(int group_size, const int *shot_ids, F f);

    // ---- one cufd call (run): its state and its passes -------------------------------------------------------------------
    struct Call {  // what every pass of one call shares; ONE snapshot of the kernel options
        KernelOptions opt;
        hipStream_t st = nullptr;
        bool if_res = false, with_adj = false, to_store = false;
        int group_size = 0;
        const int *shot_ids = nullptr;
        std::vector<float> stf_rows;  // tapered source traces of the call's shots (host)
        float src_scale = 0.0f;
        int n_probe = 0;              // HIP-event pairs handed out in the running backward pass
        int ph_every = 0;             // > 0: the call accumulates the pseudo-Hessian on every ph_every-th forward step (armed, calc_id 0 / 1)
        std::chrono::steady_clock::time_point t_begin;  // begin_call, for total_ms
    };
    // How run, born and adjoint_exact open and close a call (session_run.cpp).  The entry point holds the lock and has made the refusals
    // that must leave everything untouched; what differs between them (if_res, with_adj, to_store, ph_every, options it overrides,
    // last_exact_ / last_batched_, whether the observed store is touched: obs_begin) it sets on the Call it gets back.
    Call begin_call(hipStream_t ext_stream, int group_size, const int *shot_ids);
    void check_shot_ids(int group_size, const int *shot_ids) const;
    void obs_begin(const Call &c);
    void end_call(const Call &c, bool sync);
    // closes a timing bracket whose events ev_[a], ev_[a + 1] are recorded on st: waits for the stream, -> the time between them
    double bracket_ms(int a, hipStream_t st);
    // the components with a weight (by default the axial strain alone): f(comp, column block of the adjoint-source array), and as a mask
    // of seismogram components (bit comp)
    template <class F> void for_active(F f) const {
        for (int comp = 1; comp <= 3; comp++)
            if (geo_block_[comp] >= 0) f(comp, geo_block_[comp]);
    }
    int active_comps() const { return (geo_block_[1] >= 0 ? 2 : 0) | (geo_block_[2] >= 0 ? 4 : 0) | (geo_block_[3] >= 0 ? 8 : 0); }
    // The three dense gradients of a finalisation kernel: written in place where the caller's array lives on this device (dev = out),
    // else into grad_stage_ and copied out on the stream after the launch (host memory, another GPU)
    struct GradOut {
        float *out[3], *dev[3];
    };
    GradOut grad_out(float *gLambda, float *gMu, float *gDen) const;
    void copy_staged(const GradOut &o, hipStream_t st);
    // the call's misfit from the sums on the device, the joint weights applied; parts: also what sepfwi_get_misfit_parts reports
    void read_misfit(const Call &c, float *misfit, bool parts);
    struct GaugeDev;
    struct InjDev;
    // A shot's working set: forward state (schedule.hpp: [5 fields | 8 memories]), boundary frames (null until a gradient call needs
    // them), seismograms, residual, its slot of the quiet-map pool, its stream.  state null: there is no such lane.
    struct Lane {
        float *state = nullptr, *frame = nullptr, *syn = nullptr, *res = nullptr;
        unsigned int *quiet = nullptr;  // ShotCtx: null unless the shot runs with option quiet_skip
        hipStream_t st = nullptr;
    };
    // lane k of the stream schedule (0: the session's own arrays on the call's stream; k >= 1: xl_[k]) and of the batched schedule (the
    // arenas ba_ at their constant strides), with the backward block of a batch lane (null: none)
    Lane stream_lane(int k, hipStream_t call_st = nullptr) const;
    Lane batch_lane(int k, hipStream_t call_st = nullptr) const;
    float *batch_bwd(int k) const;
    size_t frame_lane_len() const { return (size_t)par_.nSteps * 5 * (size_t)g_.frame_len; }
    struct ShotCtx : Lane {  // one shot of the call in the lane it runs in
        int is, id, nrec, comps;
        int nres;               // row length of `res`: nrec, or C nrec for a joint misfit (geophone.hpp)
        const float *obs_c[4];  // joint misfit: the observed gathers of the active components, by component id
        const Shot *sh;
        const int *rec;
        const float *stf_s, *d_obs;
        const float *sens;  // directional sensitivities of this shot's channels (device) or null
        const GaugeDev *gauge;  // parameter key das_gauge_length (G > 1): the channels' taps (device), else null
        const InjDev *ginj;     // ... and their adjoint plan (gradient calls)
        bool scratch;
        LineRec line;
        // (Lane::quiet, option quiet_skip: the lane's four quiet-segment maps -- forward v, forward s, adjoint v, adjoint s -- or null)
        float *ph;            // armed call: the pseudo-Hessian accumulator set of the shot's stream lane, else null
        Fields fld;           // views of Lane::state
        PmlMem mem;
    };
    struct BwdLane {  // stream + backward-pass memory variables + adjoint fields + imaging accumulators
        hipStream_t s;
        PmlMem bm;
        Fields adj;
        ImgAcc acc;
    };
    void prepare_media(Call &c, const float *Lambda, const float *Mu, const float *Den);
    void prepare_buffers(Call &c, const float *stf);
    ShotCtx make_ctx(const Call &c, int is, const Lane &lane, bool with_obs = true);
    static constexpr int kQuietSlots = kMaxLanes + 64;  // one per stream lane and batch lane (option batch_f <= 64)
    unsigned int *quiet_slot(int slot) const { return quiet_pool_ + (size_t)slot * 4 * (size_t)g_.qn; }
    bool quiet_wanted(const Call &c, const ShotCtx &x) const { return c.opt.quiet_skip != 0 && !joint_ && (x.nrec == 0 || (x.line.n > 0 && c.opt.line_fuse != 0)); }
    // the residual of a fused line enters inside the field kernels -- unless the misfit is a joint one, whose adjoint source goes through the plan
    bool inject_inline(const Call &c, const ShotCtx &x) const { return x.line.n > 0 && c.opt.line_fuse != 0 && !joint_; }
    float *syn_of(const ShotCtx &x, int comp) const { return x.syn + (size_t)comp * data_len_; }
    bool forward_inline(const Call &c, const ShotCtx &x) const { return x.line.n > 0 && !(x.comps & 1) && c.opt.line_fuse != 0; }
    // forward pass of one shot, stream form (libCUFD.cu:268-332)
    void forward_init(const ShotCtx &x);
    void forward_step(const Call &c, const ShotCtx &x, int it, bool inl);
    void record_column(const ShotCtx &x, int column);
    void record_background(const ShotCtx &x, int column);  // session_born.cpp (if_envelope_misfit, robust_misfit)
    const GaugeDev &gauge_taps(const ShotCtx &x);  // a gauge shot's taps on the device, built on first use (das_gauge.hpp)
    void residual(const ShotCtx &x);
    GeoResShot geo_res_shot(const ShotCtx &x) const;  // joint misfit: what the residual kernel needs of one shot (geophone.hpp)
    void residual_batch(const Call &c, const std::vector<ShotCtx> &cx, int nb);
    void residual_conditioned(const Call &c, const ShotCtx &x);        // session_data.cpp: the same through the conditioning chain
    void adjoint_source_conditioned(const Call &c, const ShotCtx &x);  // -C^T Z C (J v) from the shot's scattered gather (if_win / filter)
    // what a forward pass leaves behind, by kind of call
    void after_forward(Call &c, const ShotCtx &x);
    void export_gathers(const Call &c, const ShotCtx &x);
    void scratch_dumps(const Call &c, const ShotCtx &x);
    // backward pass of one shot, stream form (libCUFD.cu:500-675)
    void backward_init(const BwdLane &L);
    void backward_step(Call &c, const ShotCtx &x, const BwdLane &L, int it);
    void inject_column(const ShotCtx &x, const BwdLane &L, const float *res_t);
    Grid step_grid(const KernelOptions &opt, int it) const;  // the grid with backward step it's imaging weight (option img_every)
    void backward(Call &c, const ShotCtx &x);
    // the exact transposed time loop of one shot and its finalisation on Omega (session_exact.cpp); the persistent loop is not used
    void backward_exact(Call &c, const ShotCtx &x, bool src_gather = false);
    void write_outputs_exact(Call &c, float *g_Lambda, float *g_Mu, float *g_Den);
    void write_stf_exact(Call &c, float *g_stf);
    // the same pass as ONE persistent launch (option bwd_fuse = 4; kernels.hip k_bwd_persist)
    struct Persist;
    bool persist_ready(const Call &c, const ShotCtx &x);
    bool persist_prepare(Persist &k, const KernelOptions &opt, int nshots);
    bool backward_persistent(Call &c, const ShotCtx &x, const BwdLane &L);
    bool batched_backward_persistent(Call &c, const std::vector<ShotDev> &tab, int first, int nbb);
    ShotDev shot_dev(const Call &c, const ShotCtx &x) const;  // what the loop's record of a shot and the batched schedule's share
    bool persist_launch(Persist &k, Call &c, PersistArgs &a, hipStream_t st);
    const InjArgs *persist_inject(const Call &c, const ShotCtx &x, hipStream_t st);
    InjDev &inj_dev(const ShotCtx &x);
    void persist_demote(Persist &k, const std::string &why, int retry_in);
    void persist_check_pass(Persist &k);
    const Event *probe_pair(Call &c, int it);
    void collect_probes(Call &c);
    // the two schedules of a call's shots
    void run_streams(Call &c, int n_lanes);
    // batched schedule (session_batched.cpp)
    void run_batched(Call &c, const Schedule &s);
    ShotCtx batch_ctx(const Call &c, int is, int Bf, bool with_obs);
    std::vector<ShotDev> batch_table(const Call &c, int Bf, int Bb);
    struct SubBatch : SubRange {  // a sub-batch (schedule.hpp) and the stream it runs on
        hipStream_t st;
    };
    std::vector<SubBatch> batch_streams(hipStream_t st, const std::vector<ShotFacts> &shots, int ns);
    void batch_join(hipStream_t st, int ns);
    void batched_forward(Call &c, const std::vector<ShotDev> &tab, int is0, int nb, int split, const std::vector<ShotCtx> &cx);
    void batched_backward(Call &c, const std::vector<ShotDev> &tab, int first, int nbb, int split, const ShotCtx *cx);
    void ph_begin(Call &c, int nsets);  // armed call: the accumulator sets of its lanes / sub-batch streams, zeroed on the call's stream
    PhAcc ph_acc(const float *set) const { float *s = const_cast<float *>(set); return PhAcc{s, s + cells_, s + 2 * cells_}; }
    void write_outputs(Call &c, float *misfit, float *grad_Lambda, float *grad_Mu, float *grad_Den, float *grad_stf);

    std::string para_fname_;
    int gpu_id_;
    std::string para_text_, survey_text_;
    Params par_;
    Survey survey_;
    Grid g_{};
    std::mutex mu_;
    // Ownership (device_alloc.hpp): every device block of the session is a buffer booked in device_bytes_ at its real size while it is
    // held (sepfwi_stats.device_bytes).  Members are destroyed in reverse order of declaration: the buffers first, the events and streams
    // after them, the conditioner's FFT plans last -- ~Session only waits for the device.
    long long device_bytes_ = 0;
    template <class T> DevBuf<T> dev(size_t n) { return DevBuf<T>(&device_bytes_, n); }
    // a host vector as a device block of its own (at least one element: the kernels take the pointer of an empty table too)
    template <class T> DevBuf<T> upload(const std::vector<T> &v) {
        DevBuf<T> b = dev<T>(std::max<size_t>(1, v.size()));
        if (!v.empty()) HIP_OK(hipMemcpy(b.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return b;
    }
    // data conditioning (any live conditioning key, Params::first_live_key): the kernels' scratch and the hipFFT work space
    std::unique_ptr<Conditioner> cond_;
    Stream own_stream_;
    Event ev_order_;
    static constexpr int kProbePairs = 64;
    Event probe_ev_[2 * kProbePairs];
    Event ev_[4];
    PinBuf<float> h_io_;
    DevBuf<float> stf_grad_{&device_bytes_}, frame_;
    std::vector<DevBuf<char>> allocs_;  // the constructor's blocks (dalloc): what state_, media_ ... below are views of

    size_t cells_ = 0, data_len_ = 0;
    // joint DAS + geophone misfit (parameter keys misfit_w_*; geophone.hpp): on?, number of active components, the column block of
    // each in the adjoint-source array (-1: weight 0), the length of a residual buffer (data_len_ x the active components), the sums
    // sum r_c^2 on the device (by comp - 1), the batched residual kernel's table, the backward twin of the batched schedule's shot
    // table (no fused lines, no generic receivers: the plan serves every shot), what the last call left for sepfwi_get_misfit_parts
    bool joint_ = false;
    int geo_ncomp_ = 1, geo_block_[4] = {-1, -1, -1, 0};
    size_t res_len_ = 0;
    double *geo_sums_ = nullptr;
    std::vector<GeoResShot> geo_res_tab_;
    double parts_[3] = {0.0, 0.0, 0.0};
    // diagonal pseudo-Hessian (pseudo_hessian.hpp): armed with this stride (0: not armed); one accumulator set [E_lam | E_mu | E_rho]
    // per concurrently running forward lane or sub-batch stream, allocated on first use; how many the running call uses; the result
    // of the most recent armed call, three dense (nz, nx) arrays, and whether there is one
    int ph_every_ = 0;
    int ph_nsets_ = 0;
    bool ph_valid_ = false;
    // Born modelling (born.hpp), allocated on the first Born call: [5 scattered fields | their 8 C-PML memories | 5 perturbed-media
    // arrays] and the staging of a perturbation that does not live on this device
    DevBuf<float> born_stage_, born_;
    // envelope misfit (parameter key if_envelope_misfit): the time-major BACKGROUND axial-strain gather of the shot a Born call is
    // running, allocated by the first product under the key; a third [rec][it] scratch gather and a sum of their own for that product
    // and the data-space entry points, allocated on first use
    DevBuf<float> born_bg_, xpose3_;
    DevBuf<double> data_acc_;
    DevBuf<float> ph_out_, ph_set_[kPhMaxSets];
    DevBuf<float> inj_val_{&device_bytes_};
    // gauge channels (parameter key das_gauge_length): per shot its taps (device copies, built on first use); the batched schedule's
    // side table of the call's shots (GaugeShotDev, indexed like d_shots_) and its host copy
    struct GaugeDev {
        DevBuf<int> start, cell, field;
        DevBuf<float> w;
    };
    DevBuf<GaugeShotDev> d_gauge_{&device_bytes_};
    std::vector<GaugeShotDev> gauge_tab_;
    std::map<int, GaugeDev> gauge_;
    // adjoint-source injection inside the loop for shots whose receivers are not a fused line: the plan of each such shot (device
    // copies, built on first use) and the pass's residual folded per target cell [nSteps][ntgt] (inj_val_)
    struct InjDev {
        DevBuf<int> lookup, tgt_start, ent_rec;
        DevBuf<int> tgt_cell, tgt_field;  // gauge shots: per target its flat cell and field (k_inject_gauge)
        DevBuf<InjSeg> segs;
        DevBuf<float> ent_w;
        std::vector<int> target_segs;       // row segments (z * nseg + xs) that hold target cells
        DevBuf<unsigned char> tile_has;     // per tile of the tiling numbered tile_gen: owns target cells?
        InjArgs h_args{};                   // what the kernel reads through PersistArgs::injp ...
        DevBuf<InjArgs> d_args;             // ... and its device copy
        int ntgt = 0, tile_gen = -1;
    };
    std::map<int, InjDev> inj_;
    // persistent backward time loop: the tiling in use, its device copy, synchronisation words, what the census of the grid said
    struct Persist {
        explicit Persist(bool multi_shot) : multi(multi_shot) {}
        const bool multi;  // the batched schedule's loop: the multi-shot kernel instance, also for a sub-batch of one
        PersistPlan plan;
        DevBuf<uint32_t> d_seg;
        DevBuf<TileHdr> d_hdr;
        DevBuf<unsigned int> d_sync;  // [nwg x 32 flag words | 8 band XCC ids | arrived | err]
        DevBuf<unsigned long long> d_qnbr;  // quiet variant: stencil neighbours of every row segment inside its tile (persist_plan.hpp)
        DevBuf<float> d_stf;          // (d_stf and h_err are kept across tilings, the four above belong to one)
        PinBuf<int> h_err;
        int nwg = 0, threads = 0, lmask = 0, lmask_req = -1, wpc = 0, strip_w = 0, order = -1, wx = -1, wxp = -1, wz = -1, snake = -1, nshots = 0;
        size_t lds_bytes = 0;
        int state = -1;                  // -1 not examined for this configuration, 0 the two-launch step is used, 1 ready
        std::string why;                 // when state == 0
        int plan_gen = 0;                // counts the tilings built (what depends on one is rebuilt when it changes)
        int retry_in = 0, aborts = 0;    // passes until the loop is tried again after a start rendezvous that failed; how often it did
    } pk_ms_{true}, pk_{false};  // the shots of a backward sub-batch in one launch (batched schedule) / one shot per launch (stream schedule)
    std::unique_ptr<ObservedStore> obs_;
    // extra forward lanes (lane 0 = state_/frame_/syn_/res_ on the call's stream): stream, join event, fields + memories, frames,
    // seismograms, residual
    struct XLane {
        Stream stream;
        Event join;
        DevBuf<float> state, frame, syn, res;
    };
    XLane xl_[kMaxLanes];
    void ensure_lane_stream(XLane &L);
    // batched mode: lanes of per-shot state (forward: fields + memories, frames, seismograms, residual; backward: memories,
    // adjoint fields, accumulators; batch_lane, batch_bwd) and the device tables of the call's shots and source rows
    DevBuf<float> d_stf_{&device_bytes_};
    DevBuf<GeoResShot> d_geo_res_{&device_bytes_};
    DevBuf<ShotDev> d_shots_bwd_{&device_bytes_}, d_shots_{&device_bytes_};
    struct BatchArenas {  // the lanes of one kind at a constant stride (ensure_batch)
        explicit BatchArenas(long long *tally) : state(tally), syn(tally), res(tally), frame(tally), bwd(tally) {}
        DevBuf<float> state, syn, res, frame, bwd;
    } ba_{&device_bytes_};
    bool last_batched_ = false;
    float *state_ = nullptr, *media_ = nullptr, *acc_buf_ = nullptr, *in_stage_ = nullptr, *grad_stage_ = nullptr;
    float *syn_ = nullptr, *res_ = nullptr, *xpose_ = nullptr;
    double *scal_ = nullptr;
    unsigned int *cp2_bits_ = nullptr;
    int *rec_idx_ = nullptr;
    float *sens_ = nullptr;  // directional DAS sensitivities (3 per channel) or null
    // data conditioning: per-channel windows and weights (3 per channel: start, end, weight; same offsets as rec_idx_), a second
    // [rec][it] scratch gather
    bool cond_on_ = false;
    float *win_ = nullptr, *xpose2_ = nullptr;
    std::vector<int> rec_off_;
    std::vector<double> fk_delta_;  // parameter key fk_slowness: the channel spacing [m] of every shot (host_checks.hpp), filled at creation
    Fields fld_{}, adj_{};
    PmlMem mem_{};
    Media md_{};
    PmlCoef pc_{};
    ImgAcc acc_{};
    unsigned int *quiet_pool_ = nullptr;  // kQuietSlots x 4 maps of Grid::qn words (Fields::q)
    // What a call counts (sepfwi_stats): begin_call starts every call from CallStats{} -- a new counter cannot carry over.
    struct CallStats {
        double fwd_ms = 0, bwd_ms = 0, probe_us = 0;
        long long fwd_steps = 0, bwd_steps = 0, launches = 0, persist_steps = 0, probe_calls = 0;
        long long quiet_active = 0, quiet_total = 0;
        unsigned int *quiet_last = nullptr;  // maps of the shot whose forward pass started last in this call
        bool exact = false;                  // the call's backward passes are exact ones (loop_status)
    } cs_;
    double total_ms_ = 0;
    int last_shots_ = 0, last_calc_ = -1;
};

// The registry hands out shared ownership: a session that another thread is still running survives being replaced
// (parameter file rewritten) or released.
std::shared_ptr<Session> get_session(const std::string &para_fname, int gpu_id);
std::shared_ptr<Session> find_session(const std::string &para_fname, int gpu_id);
void release_all_sessions();
void invalidate_observed_all();

}  // namespace sepfwi
