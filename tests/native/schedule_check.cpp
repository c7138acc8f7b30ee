// CPU-only check of the schedule of a call, the sub-batches of a batch and the lane layouts (csrc/schedule.cpp, schedule.hpp), built with
// -fsanitize=address,undefined by tests/test_sanitizers.py.
//   (a) plan_schedule against the arithmetic it was lifted from, kept here word for word as the yardstick (old_schedule below), over a
//       dense sweep of array sizes, group sizes, call kinds, options and caps of the observed store;
//   (b) the grids that the comment in Session::run names, their padded array sizes worked out here as Session::init_grid /
//       alloc_arrays do it: how many backward passes fit the budget together;
//   (c) sub_ranges: non-empty, contiguous, covering, each range with the facts of exactly its shots;
//   (d) the layout views against the offsets they replace.
// Prints "OK <cases of (a)> ..." or the first difference.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../sep-2023_amd/csrc/schedule.hpp"

using namespace sepfwi;

struct Opt {  // the options the schedule reads (csrc/kernels.hpp KernelOptions)
    int batch = 2, batch_f = 0, batch_b = 0, batch_mb = 200, bwd_fuse = 4, pair_fwd = 1, fwd_lanes = 3, batch_split = 2;
};

// ObservedStore::max_group with a budget that holds `fit` gathers (fit <= 0: no budget)
static int max_group(int fit, int want) { return fit <= 0 ? want : std::max(1, std::min(fit, want)); }

// THE YARDSTICK: Session::run and Session::run_streams as they chose the schedule before schedule.cpp existed (the statements in
// their order; c.opt -> opt, obs_->max_group(bytes, want) -> max_group(fit, want)).  Not the code under test: never "simplified".
struct Old {
    bool batched;
    int Bf, Bb, n_lanes, ns_full;
};
static Old old_schedule(size_t cells_, const Opt &opt, int group_size, bool with_adj, bool if_res, int fit) {
    const int kMaxLanes = 4;
    Old o{};
    const double arr_mb = (double)cells_ * sizeof(float) / 1.0e6, budget = (double)opt.batch_mb;
    int Bf = (int)((budget / arr_mb - 5.0) / 5.0), Bb = (int)((budget / arr_mb - 5.0) / 15.0);
    const int bb_min = opt.bwd_fuse == 4 ? 3 : 2;
    const bool batched = opt.bwd_fuse != 0 && group_size >= 1 &&
                         (opt.batch == 1 || (opt.batch == 2 && (with_adj ? Bb >= bb_min : Bf >= 8)));  // forward-only calls: streams until kernels are launch-bound
    o.batched = batched;
    if (batched) {
        if (opt.batch_f > 0) Bf = opt.batch_f;
        if (opt.batch_b > 0) Bb = opt.batch_b;
        Bf = std::max(1, std::min(std::min(Bf, 32), group_size));
        if (if_res) Bf = max_group(fit, Bf);
        Bb = std::max(1, std::min(Bb, Bf));
        if (!opt.pair_fwd) Bf = Bb = 1;
        o.Bf = Bf;
        o.Bb = Bb;
        o.ns_full = std::max(1, std::min(std::min(opt.batch_split, (int)kMaxLanes - 1), Bf));  // batched_forward, for a full batch
    } else {
        int n_lanes = opt.pair_fwd ? opt.fwd_lanes : 1;
        n_lanes = std::max(1, std::min(std::min(n_lanes, group_size), (int)kMaxLanes));
        if (if_res) n_lanes = max_group(fit, n_lanes);
        o.n_lanes = n_lanes;
    }
    return o;
}

static Schedule new_schedule(size_t cells, const Opt &opt, int group_size, bool with_adj, bool if_res, int fit, int *cap_calls = nullptr) {
    ScheduleIn in;
    in.array_bytes = cells * sizeof(float);
    in.batch = opt.batch;
    in.batch_f = opt.batch_f;
    in.batch_b = opt.batch_b;
    in.batch_mb = opt.batch_mb;
    in.bwd_fuse = opt.bwd_fuse;
    in.pair_fwd = opt.pair_fwd;
    in.fwd_lanes = opt.fwd_lanes;
    in.batch_split = opt.batch_split;
    in.group_size = group_size;
    in.with_adj = with_adj;
    in.if_res = if_res;
    return plan_schedule(in, [&](int want) {
        if (cap_calls) ++*cap_calls;
        return max_group(fit, want);
    });
}

static bool same(const Old &o, const Schedule &s) {
    if (o.batched != s.batched) return false;
    return o.batched ? (o.Bf == s.Bf && o.Bb == s.Bb && o.ns_full == s.split && s.lanes == 0) : (o.n_lanes == s.lanes && s.Bf == 0 && s.Bb == 0 && s.split == 0);
}

// one padded array of a (nz x nx)-cell problem with nPml absorbing cells on every side: Session::init_grid (pitch: rows padded to 64
// floats; the nPad dead rows are not stored) and alloc_arrays (4 spare rows)
static size_t padded_cells(int nz, int nx, int nPml) {
    const int nzc = nz + 2 * nPml, nx_pad = nx + 2 * nPml, pitch = ((nx_pad + 63) / 64) * 64;
    return (size_t)(nzc + 4) * (size_t)pitch;
}

static long long sweep() {
    long long cases = 0;
    std::vector<size_t> sizes;
    for (int k = 0; k < 32; k++) sizes.push_back((size_t)(0.05e6 / 4.0 * std::pow(800.0, k / 31.0)));  // 0.05 ... 40 MB, geometric
    const int grids[6][2] = {{500, 2000}, {500, 1500}, {700, 1000}, {300, 2000}, {500, 1000}, {101, 201}};
    for (auto &g : grids) sizes.push_back(padded_cells(g[0], g[1], 32));
    int rot = 0;
    for (size_t cells : sizes)
        for (int group = 0; group <= 40; group++)
            for (int kind = 0; kind < 3; kind++)  // observe (no residual), misfit, gradient
                for (int batch = 0; batch <= 2; batch++)
                    for (int fuse = 0; fuse <= 4; fuse += 2)
                        for (int bf = 0; bf <= 5; bf++)
                            for (int bb = 0; bb <= 5; bb++)
                                for (int fit = 0; fit <= 8; fit++, rot++) {  // 0: no budget
                                    Opt opt;
                                    opt.batch = batch;
                                    opt.bwd_fuse = fuse;
                                    opt.batch_f = bf;
                                    opt.batch_b = bb;
                                    opt.pair_fwd = rot % 5 != 0;          // the options without a public name: rotated through
                                    opt.fwd_lanes = 1 + rot % 4;
                                    opt.batch_split = 1 + (rot / 4) % 3;
                                    opt.batch_mb = (rot % 7 == 0) ? 100 : 200;
                                    const bool with_adj = kind == 2, if_res = kind >= 1;
                                    const Old o = old_schedule(cells, opt, group, with_adj, if_res, fit);
                                    int calls = 0;
                                    const Schedule s = new_schedule(cells, opt, group, with_adj, if_res, fit, &calls);
                                    if (!same(o, s) || calls != (if_res ? 1 : 0)) {
                                        printf("FAIL sweep: cells %zu group %d kind %d batch %d bwd_fuse %d batch_f %d batch_b %d fit %d: old %d %d %d %d %d, new %d %d %d %d %d, cap asked %d times\n",
                                               cells, group, kind, batch, fuse, bf, bb, fit, o.batched, o.Bf, o.Bb, o.ns_full, o.n_lanes, s.batched, s.Bf, s.Bb, s.split,
                                               s.lanes, calls);
                                        return -1;
                                    }
                                    cases++;
                                }
    return cases;
}

// (b) a gradient call of many shots with the default options: how many backward passes share a launch
static int named_grids(std::string *report) {
    struct G {
        const char *name;
        int nz, nx, shots, want_bb;
        bool want_batched;
    };
    // 2000x300: (200 MB / 3.109 MB - 5) / 15 = 3.96 -> three passes, not the four an earlier comment in Session::run gave it
    const G grids[] = {{"2000x500", 500, 2000, 32, 2, false}, {"1500x500", 500, 1500, 32, 3, true}, {"1000x700", 700, 1000, 32, 3, true},
                       {"2000x300", 300, 2000, 32, 3, true},  {"1000x500", 500, 1000, 32, 5, true}, {"101x201 x 19 shots", 101, 201, 19, 19, true}};
    for (const G &g : grids) {
        const size_t cells = padded_cells(g.nz, g.nx, 32);
        Opt opt, always;
        always.batch = 1;  // the batch sizes also where the default takes the stream schedule
        const Schedule forced = new_schedule(cells, always, g.shots, true, true, 0), s = new_schedule(cells, opt, g.shots, true, true, 0);
        const double mb = (double)cells * 4.0 / 1.0e6;
        char line[256];
        snprintf(line, sizeof line, "# %-20s array %.3f MB  (budget / array - 5) / 15 = %.3f  Bf %d Bb %d  default: %s\n", g.name, mb, (200.0 / mb - 5.0) / 15.0,
                 forced.Bf, forced.Bb, s.batched ? "batched" : "streams");
        *report += line;
        if (forced.Bb != g.want_bb || s.batched != g.want_batched) {
            printf("FAIL grid %s: Bb %d (want %d), batched %d (want %d)\n", g.name, forced.Bb, g.want_bb, (int)s.batched, (int)g.want_batched);
            return -1;
        }
        if (g.shots == 19 && (s.Bf != 19 || s.Bb != 19)) {
            printf("FAIL the notebook problem does not run all its shots at once: Bf %d Bb %d\n", s.Bf, s.Bb);
            return -1;
        }
    }
    return 0;
}

static int ranges(unsigned seed) {
    std::mt19937 rng(seed);
    for (int nb = 1; nb <= 64; nb++)
        for (int ns = 1; ns <= 3; ns++)
            for (int rep = 0; rep < 8; rep++) {
                std::vector<ShotFacts> f((size_t)nb);
                for (ShotFacts &x : f) {
                    x.general = rng() % 4 == 0;
                    x.gauge = rng() % 3 == 0 ? (int)(rng() % 50) : 0;
                }
                const std::vector<SubRange> r = sub_ranges(f, ns);
                if ((int)r.size() != std::min(ns, nb)) return 1;
                int at = 0;
                for (size_t q = 0; q < r.size(); q++) {
                    if (r[q].q != (int)q || r[q].a0 != at || r[q].a1 <= r[q].a0 || r[q].n() != r[q].a1 - r[q].a0) return 2;  // contiguous, non-empty
                    if (r[q].a0 != (int)((long long)nb * (long long)q / (long long)r.size()) || r[q].a1 != (int)((long long)nb * (long long)(q + 1) / (long long)r.size())) return 3;
                    bool general = false;
                    int gauge = 0;
                    for (int k = r[q].a0; k < r[q].a1; k++) {
                        general = general || f[k].general;
                        gauge = std::max(gauge, f[k].gauge);
                    }
                    if (general != r[q].general || gauge != r[q].gauge) return 4;
                    at = r[q].a1;
                }
                if (at != nb) return 5;  // covers [0, nb)
            }
    if (sub_ranges(std::vector<ShotFacts>(5), 0).size() != 1 || sub_ranges(std::vector<ShotFacts>(5), -3).size() != 1) return 6;  // an option below 1: one range
    return 0;
}

static int layouts() {
    std::vector<float> block(18 * 7);
    float *b = block.data();
    const size_t n = 7;
    const Fields f = fields_at(b, n);
    const PmlMem m = mem_at(state_mem(b, n), n);
    const Fields a = fields_at(own_adj(b, n), n);
    if (f.vz != b || f.vx != b + n || f.szz != b + 2 * n || f.sxx != b + 3 * n || f.sxz != b + 4 * n || f.q != nullptr) return 1;
    if (m.dvz_dz != b + 5 * n || m.dvz_dx != b + 6 * n || m.dvx_dz != b + 7 * n || m.dvx_dx != b + 8 * n || m.dszz_dz != b + 9 * n || m.dsxz_dx != b + 10 * n ||
        m.dsxz_dz != b + 11 * n || m.dsxx_dx != b + 12 * n)
        return 2;
    if (a.vz != b + 13 * n || a.sxz != b + 17 * n) return 3;
    if (bwd_adj(b, n) != b + 8 * n || bwd_acc(b, n) != b + 13 * n) return 4;
    const ImgAcc c = acc_at(bwd_acc(b, n), n);
    if (c.lam != b + 13 * n || c.mu != b + 14 * n || c.xz != b + 15 * n || c.a != b + 16 * n || c.b != b + 17 * n) return 5;
    const Media md = media_at(b, n);
    if (md.lam != b || md.mu != b + n || md.ave_mu != b + 2 * n || md.byc_a != b + 3 * n || md.byc_b != b + 4 * n || md.rho != b + 5 * n) return 6;
    if (kStateArrays != 13 || kOwnArrays != 18 || kBwdArrays != 18 || kBwdZeroed != 13 || kAccArrays != 5 || kMaxLanes != 4) return 7;
    return 0;
}

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    std::string report;
    if (named_grids(&report) != 0) return 1;
    if (const int rc = ranges(seed)) {
        printf("FAIL sub_ranges: code %d\n", rc);
        return 1;
    }
    if (const int rc = layouts()) {
        printf("FAIL layouts: code %d\n", rc);
        return 1;
    }
    const long long cases = sweep();
    if (cases < 0) return 1;
    printf("OK %lld schedules equal the yardstick's\n%s", cases, report.c_str());
    return 0;
}
