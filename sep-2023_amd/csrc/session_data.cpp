// session_data.cpp -- Session::data_misfit / data_gn: the misfit of the parameter file as an operator on gathers (sepfwi_data_misfit,
// sepfwi_data_gn), with no wave propagation.
//
// Both take RAW axial-strain gathers, [nrec_i][nSteps] shot after shot like born()'s d_ett, host or device, and run them through the code a
// gradient call or a Gauss-Newton product runs between its two transpositions (Session::misfit_chain, Session::gn_chain):
//   data_misfit   the file's misfit of (obs, syn) and the raw-space adjoint source a = -d misfit / d syn: C^T Z (C obs - C syn) under an L2
//                 file, the adjoint source of the normalised cross-correlation under if_cross_misfit, C^T D^T Z (e(C obs) - e(C syn)) under
//                 if_envelope_misfit.  Under if_src_update the matching filter is computed from the call's own (C obs, C syn), shot by shot,
//                 as a gradient call computes it; the misfit is that of the updated synthetics and a is taken with the filter held fixed
//                 (nothing is carried from one shot or call to the next).
//   data_gn       the Gauss-Newton operator of the misfit in data space at syn: C^T Z C d, or C^T D^T Z D C d under if_envelope_misfit.
//                 Refused under if_cross_misfit and if_src_update (not a least-squares misfit of the data), as the products are.
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

// the third [rec][it] scratch gather and the sum of the data-space entry points (and of the envelope product of Session::born)
void Session::ensure_data_scratch() {
    if (!xpose3_) xpose3_ = dev<float>(data_len_);
    if (!data_acc_) data_acc_ = dev<double>(1);
}

void Session::data_misfit(float *misfit, float *adj, const float *obs, const float *syn, int group_size, const int *shot_ids, hipStream_t ext_stream) {
    std::lock_guard<std::mutex> lock(mu_);
    if (joint_) throw std::invalid_argument("data_misfit: not defined for a joint misfit (misfit_w_*): it is a misfit of axial-strain gathers alone");
    check_shot_ids(group_size, shot_ids);
    HIP_OK(hipSetDevice(gpu_id_));
    hipStream_t st = ext_stream ? ext_stream : own_stream_.get();
    if (!ext_stream) order_after_null_stream(st);
    ensure_data_scratch();
    double *acc = data_acc_.get();
    HIP_OK(hipMemsetAsync(acc, 0, sizeof(double), st));
    const int nSteps = par_.nSteps;
    size_t off = 0;
    for (int is = 0; is < group_size; is++) {
        const int id = shot_ids[is], nrec = survey_.shots[id].nrec;
        const size_t cnt = (size_t)nrec * nSteps, bytes = cnt * sizeof(float);
        if (cnt == 0) continue;
        if (cond_on_) {  // the observed gather is kept conditioned (obs_store.cpp): C obs, then the chain on the raw synthetic gather
            HIP_OK(hipMemcpyAsync(xpose3_.get(), obs + off, bytes, hipMemcpyDefault, st));
            condition_gather(st, xpose3_.get(), id, nrec);
            HIP_OK(hipMemcpyAsync(xpose_, syn + off, bytes, hipMemcpyDefault, st));
            misfit_chain(st, xpose3_.get(), id, nrec, acc);
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
        off += cnt;
    }
    double sum = 0.0;
    HIP_OK(hipMemcpyAsync(&sum, acc, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const float mf = (float)(0.5 * sum);  // as read_misfit halves the total
    if (misfit) HIP_OK(hipMemcpy(misfit, &mf, sizeof(float), hipMemcpyDefault));
}

void Session::data_gn(float *out, const float *syn, const float *d, int group_size, const int *shot_ids, hipStream_t ext_stream) {
    std::lock_guard<std::mutex> lock(mu_);
    if (par_.if_cross_misfit || par_.if_src_update)
        throw std::invalid_argument(std::string("data_gn: not defined under ") + (par_.if_cross_misfit ? "if_cross_misfit" : "if_src_update") +
                                    " (not a least-squares misfit of the data); if_win, filter and if_envelope_misfit are served");
    if (joint_) throw std::invalid_argument("data_gn: not defined for a joint misfit (misfit_w_*): it is a misfit of axial-strain gathers alone");
    check_shot_ids(group_size, shot_ids);
    HIP_OK(hipSetDevice(gpu_id_));
    hipStream_t st = ext_stream ? ext_stream : own_stream_.get();
    if (!ext_stream) order_after_null_stream(st);
    if (par_.if_envelope_misfit) ensure_data_scratch();
    const int nSteps = par_.nSteps;
    size_t off = 0;
    for (int is = 0; is < group_size; is++) {
        const int id = shot_ids[is], nrec = survey_.shots[id].nrec;
        const size_t cnt = (size_t)nrec * nSteps, bytes = cnt * sizeof(float);
        if (cnt == 0) continue;
        HIP_OK(hipMemcpyAsync(xpose_, d + off, bytes, hipMemcpyDefault, st));
        if (cond_on_) {
            if (par_.if_envelope_misfit) HIP_OK(hipMemcpyAsync(xpose3_.get(), syn + off, bytes, hipMemcpyDefault, st));
            gn_chain(st, id, nrec, 1.0f);
            HIP_OK(hipMemcpyAsync(out + off, xpose2_, bytes, hipMemcpyDefault, st));
        } else {  // Z alone: sample 0 of every trace zeroed
            HIP_OK(hipMemset2DAsync(xpose_, (size_t)nSteps * sizeof(float), 0, sizeof(float), (size_t)nrec, st));
            HIP_OK(hipMemcpyAsync(out + off, xpose_, bytes, hipMemcpyDefault, st));
        }
        off += cnt;
    }
    HIP_OK(hipStreamSynchronize(st));
}

}  // namespace sepfwi
