// model_call.hpp -- the host side that every model-space operator shares (param_maps, regularizer, smoother): which device a call's
// arrays live on, the calling thread's current device switched and restored, host arrays staged for the length of the call, and the
// grow-only device workspaces the operators keep between calls.  The session's own staging (persistent stage buffers) is not this.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <utility>
#include <vector>

#include "device_alloc.hpp"

namespace sepfwi {

int ptr_device(const void *p);  // session_run.cpp: the device of a device pointer, -1 for host memory (and for NULL)

// One call of a model-space operator on arrays of n floats, in this order: see() every array, enter(), in() / out() what the kernels
// take, the launches, finish().  Nothing touches HIP before the first see(): an entry point validates and takes its early returns
// first.  Each pointer's device is asked for once per call.
class ModelCall {
  public:
    // device_only: an array in host memory (or a NULL one) is refused, nothing is ever staged (the parameterisation maps)
    ModelCall(const char *who, size_t n, hipStream_t st, bool device_only = false) : who_(who), n_(n), st_(st), device_only_(device_only) {}
    ~ModelCall();  // frees the staging blocks, then restores the thread's device
    ModelCall(const ModelCall &) = delete;
    ModelCall &operator=(const ModelCall &) = delete;

    // notes p's device (NULL and host memory: none); a second device is refused with "<who>: arrays live on different devices"
    void see(const void *p);
    // the call's device -- that of the first device array seen, else the thread's current one -- made current until destruction
    int enter();
    bool on_device(const void *p) { return p && device_of(p) == dev_; }
    // p itself where it lives on the call's device (and NULL for NULL), else a block of n floats held until destruction: in() copies
    // p up on the stream, out() has finish() copy the block back
    const float *in(const float *p) { return stage(const_cast<float *>(p), false); }
    float *out(float *p) { return stage(p, true); }
    // `bytes` at the device address src reach the host address dst in finish() (the regulariser's one double)
    void host_result(void *dst, const void *src, size_t bytes) { back_.push_back({dst, src, bytes}); }
    // the copies back, and one hipStreamSynchronize exactly when something was staged or a host result asked for
    void finish();

  private:
    struct Back {
        void *dst;
        const void *src;
        size_t bytes;
    };
    int device_of(const void *p);
    float *stage(float *p, bool is_out);

    std::string who_;
    size_t n_;
    hipStream_t st_;
    bool device_only_;
    int dev_ = -1, prev_ = -1;
    std::vector<std::pair<const void *, int>> seen_;
    std::vector<DevBuf<float>> staged_;
    std::vector<Back> back_;
};

// The grow-only block of `count` elements that operator `op` keeps on (dev, st) between calls; contents are never kept.  The pointer
// stays good until the same key asks for more or release_model_workspaces() (sepfwi_release_all) frees every block.
enum class ModelOp { Regularizer, Smoother };
void *model_workspace_bytes(ModelOp op, int dev, hipStream_t st, size_t bytes);
template <class T>
T *model_workspace(ModelOp op, int dev, hipStream_t st, size_t count) {
    return static_cast<T *>(model_workspace_bytes(op, dev, st, count * sizeof(T)));
}
void release_model_workspaces() noexcept;

}  // namespace sepfwi
