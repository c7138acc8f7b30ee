// schedule.hpp -- how a call's shots are scheduled and where the arrays of a lane lie.  HIP-free, as persist_plan.hpp and
// inject_plan.hpp are: tests/native/schedule_check.cpp checks all of it on the CPU.
//   plan_schedule    batched or streams, the batch sizes, the stream lanes, the sub-batches
//   sub_ranges       a batch of shots as sub-batches, each with the facts its time loops need
//   fields_at ...    the blocks of arrays a lane is made of
#pragma once
#include <cstddef>
#include <functional>
#include <vector>

#include "fwi_types.hpp"

namespace sepfwi {

constexpr int kMaxLanes = 4;  // stream lanes of a session; a batch runs as at most kMaxLanes - 1 sub-batches

// ---- the schedule of a call ---------------------------------------------------------------------------------------------------
struct ScheduleIn {
    size_t array_bytes = 0;  // one padded array of the grid
    int batch = 2, batch_f = 0, batch_b = 0, batch_mb = 200, bwd_fuse = 4, pair_fwd = 1, fwd_lanes = 3, batch_split = 2;  // the options (kernels.hpp)
    int group_size = 0;
    bool with_adj = false, if_res = false;
};
struct Schedule {
    bool batched = false;
    int Bf = 0, Bb = 0;  // batched: shots of a forward launch, of a backward launch (Bb <= Bf)
    int split = 0;       // batched: sub-batches a batch of Bf shots runs as (a smaller batch: as many as it has shots, at most)
    int lanes = 0;       // streams: forward passes side by side
};
// Batch sizes from the Infinity-Cache budget batch_mb: a forward batch keeps 5 fields per shot + 5 media arrays resident, a backward
// batch 15 arrays per shot + 5.  Where fewer than three backward passes fit (two-launch step: two) the stream schedule runs them one
// by one.  cap(want) <= want: how many observed gathers the store can hold at once (ObservedStore::max_group), asked only of a call
// that forms residuals, after the clamp to the group and before Bb follows Bf.
Schedule plan_schedule(const ScheduleIn &in, const std::function<int(int)> &cap);

// ---- a batch as sub-batches ---------------------------------------------------------------------------------------------------
struct ShotFacts {
    bool general = false;  // the shot's channels are served by the general-receiver launch of the time loop (not inside the field kernels)
    int gauge = 0;         // rows of the gauge twin's launch the shot needs: its channels (forward), its adjoint targets (backward); 0: none
};
struct SubRange {  // shots [a0, a1) of the batch, on stream q of the batch
    int q = 0, a0 = 0, a1 = 0;
    bool general = false;  // any of its shots
    int gauge = 0;         // the largest of its shots
    int n() const { return a1 - a0; }
};
// shots.size() shots as min(ns, shots.size()) (at least one) ranges [nb q / ns, nb (q + 1) / ns)
std::vector<SubRange> sub_ranges(const std::vector<ShotFacts> &shots, int ns);

// ---- the arrays of a lane, each n floats --------------------------------------------------------------------------------------
//   forward state of a lane      [5 fields | 8 C-PML memories]                      kStateArrays
//   the session's own block      [5 fields | 8 memories | 5 adjoint fields]         kOwnArrays (its accumulators: a block of their own)
//   backward block, batch lane   [8 memories | 5 adjoint fields | 5 accumulators]   kBwdArrays, the first kBwdZeroed cleared per pass
constexpr size_t kFieldArrays = 5, kMemArrays = 8, kAccArrays = 5;
constexpr size_t kStateArrays = kFieldArrays + kMemArrays, kOwnArrays = kStateArrays + kFieldArrays;
constexpr size_t kBwdZeroed = kMemArrays + kFieldArrays, kBwdArrays = kBwdZeroed + kAccArrays;
inline Fields fields_at(float *b, size_t n) { return Fields{b, b + n, b + 2 * n, b + 3 * n, b + 4 * n}; }
inline PmlMem mem_at(float *b, size_t n) { return PmlMem{b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, b + 5 * n, b + 6 * n, b + 7 * n}; }
inline Media media_at(const float *b, size_t n) { return Media{b, b + n, b + 2 * n, b + 3 * n, b + 4 * n, b + 5 * n}; }  // the session's six media arrays
inline ImgAcc acc_at(float *b, size_t n) { return ImgAcc{b, b + n, b + 2 * n, b + 3 * n, b + 4 * n}; }
inline float *state_mem(float *state, size_t n) { return state + kFieldArrays * n; }
inline float *own_adj(float *own, size_t n) { return own + kStateArrays * n; }
inline float *bwd_adj(float *bwd, size_t n) { return bwd + kMemArrays * n; }
inline float *bwd_acc(float *bwd, size_t n) { return bwd + kBwdZeroed * n; }

}  // namespace sepfwi
