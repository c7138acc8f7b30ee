// schedule.cpp -- the schedule of a call and the sub-batches of a batch (schedule.hpp).
#include "schedule.hpp"

#include <algorithm>

namespace sepfwi {

Schedule plan_schedule(const ScheduleIn &in, const std::function<int(int)> &cap) {
    Schedule s;
    const double arr_mb = (double)in.array_bytes / 1.0e6, budget = (double)in.batch_mb;
    int Bf = (int)((budget / arr_mb - 5.0) / 5.0), Bb = (int)((budget / arr_mb - 5.0) / 15.0);
    const int bb_min = in.bwd_fuse == 4 ? 3 : 2;
    s.batched = in.bwd_fuse != 0 && in.group_size >= 1 &&
                (in.batch == 1 || (in.batch == 2 && (in.with_adj ? Bb >= bb_min : Bf >= 8)));  // forward-only calls: streams until kernels are launch-bound
    if (s.batched) {
        if (in.batch_f > 0) Bf = in.batch_f;
        if (in.batch_b > 0) Bb = in.batch_b;
        Bf = std::max(1, std::min(std::min(Bf, 32), in.group_size));
        if (in.if_res) Bf = cap(Bf);
        Bb = std::max(1, std::min(Bb, Bf));
        if (!in.pair_fwd) Bf = Bb = 1;
        s.Bf = Bf;
        s.Bb = Bb;
        s.split = std::max(1, std::min(std::min(in.batch_split, kMaxLanes - 1), Bf));
    } else {
        s.lanes = std::max(1, std::min(std::min(in.pair_fwd ? in.fwd_lanes : 1, in.group_size), kMaxLanes));
        if (in.if_res) s.lanes = cap(s.lanes);
    }
    return s;
}

std::vector<SubRange> sub_ranges(const std::vector<ShotFacts> &shots, int ns) {
    const int nb = (int)shots.size();
    ns = std::max(1, std::min(ns, nb));
    std::vector<SubRange> out((size_t)ns);
    for (int q = 0; q < ns; q++) {
        SubRange &r = out[q];
        r.q = q;
        r.a0 = (int)((long long)nb * q / ns);
        r.a1 = (int)((long long)nb * (q + 1) / ns);
        for (int k = r.a0; k < r.a1; k++) {
            r.general = r.general || shots[k].general;
            r.gauge = std::max(r.gauge, shots[k].gauge);
        }
    }
    return out;
}

}  // namespace sepfwi
