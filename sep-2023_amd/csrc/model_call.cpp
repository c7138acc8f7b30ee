// model_call.cpp -- the host call path of the model-space operators (model_call.hpp).
#include "model_call.hpp"

#include <map>
#include <mutex>
#include <stdexcept>
#include <tuple>

#include "hip_check.hpp"

namespace sepfwi {

ModelCall::~ModelCall() {
    staged_.clear();
    if (prev_ >= 0) (void)hipSetDevice(prev_);
}

int ModelCall::device_of(const void *p) {
    for (const auto &s : seen_)
        if (s.first == p) return s.second;
    seen_.emplace_back(p, ptr_device(p));
    return seen_.back().second;
}

void ModelCall::see(const void *p) {
    const int d = p ? device_of(p) : -1;
    if (d < 0) {
        if (device_only_) throw std::invalid_argument(who_ + ": every array must be device memory (the host chain stays in torch)");
        return;
    }
    if (dev_ >= 0 && d != dev_) throw std::invalid_argument(who_ + ": arrays live on different devices");
    dev_ = d;
}

int ModelCall::enter() {
    HIP_OK(hipGetDevice(&prev_));
    if (dev_ < 0) dev_ = prev_;
    HIP_OK(hipSetDevice(dev_));
    return dev_;
}

float *ModelCall::stage(float *p, bool is_out) {
    if (!p || device_of(p) == dev_) return p;
    staged_.emplace_back(nullptr, n_);
    float *d = staged_.back().get();
    if (is_out)
        host_result(p, d, n_ * sizeof(float));
    else
        HIP_OK(hipMemcpyAsync(d, p, n_ * sizeof(float), hipMemcpyHostToDevice, st_));
    return d;
}

void ModelCall::finish() {
    for (const Back &b : back_) HIP_OK(hipMemcpyAsync(b.dst, b.src, b.bytes, hipMemcpyDeviceToHost, st_));
    if (!staged_.empty() || !back_.empty()) HIP_OK(hipStreamSynchronize(st_));  // results in host memory; the staging blocks go with the call
}

namespace {

struct Workspaces {
    std::mutex mu;
    std::map<std::tuple<ModelOp, int, hipStream_t>, DevBuf<unsigned char>> blocks;
};
Workspaces &workspaces() {
    static Workspaces w;
    return w;
}

}  // namespace

void *model_workspace_bytes(ModelOp op, int dev, hipStream_t st, size_t bytes) {
    Workspaces &w = workspaces();
    std::lock_guard<std::mutex> lock(w.mu);
    DevBuf<unsigned char> &b = w.blocks[std::make_tuple(op, dev, st)];
    b.ensure(bytes);
    return b.get();
}

void release_model_workspaces() noexcept {
    Workspaces &w = workspaces();
    std::lock_guard<std::mutex> lock(w.mu);
    w.blocks.clear();
}

}  // namespace sepfwi
