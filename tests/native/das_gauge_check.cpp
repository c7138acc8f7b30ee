// CPU-only check of the gauge-length channels (csrc/das_gauge.cpp, parameter key "das_gauge_length" of csrc/config.cpp), built with
// -fsanitize=address,undefined by tests/test_das_gauge_host.py.  For G = 1 ... 8 and horizontal, vertical and directional channels:
//   * the taps applied to a random field equal sum_k w_k e(p + k a), e the one-cell channel of k_record, evaluated from the definition
//     in double (1e-6 relative to the size of the terms);
//   * straight fibres give exactly 2 (odd G) / 4 (even G) taps of weights +-1/G / +-1/(2G);
//   * a uniform strain gives the same ett for every G;
//   * the plan built from the taps is the exact transpose: sum_c r_c (S v)_c == sum_t v_t (S^T r)_t (1e-12 relative) for random v, r
//     on channel sets with repeated and neighbouring channels, and its lookup / lane-mask / popcount tables find every target;
//   * members outside the grid throw, members on its edge do not; the parameter key is parsed and rejected as documented.
//   argv[1] = seed, argv[2] = number of random cases per G
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../sep-2023_amd/csrc/das_gauge.hpp"

using namespace sepfwi;

namespace {

struct Case {
    int nzc, nx, kind;  // kind 0 horizontal, 1 vertical, 2 directional along x, 3 directional along z
    float dx_dz;
    std::vector<int> zr, xr;
    std::vector<float> sens;
    bool vertical() const { return kind == 1 || kind == 3; }
    const float *s() const { return kind >= 2 ? sens.data() : nullptr; }
};

// random channels whose every member lies where a one-cell channel may lie (receiver_cells), repeated and neighbouring ones included
Case draw(std::mt19937 &rng, int G, int kind) {
    Case c;
    c.kind = kind;
    c.nzc = 2 * G + 8 + (int)(rng() % 40);
    c.nx = 2 * G + 8 + (int)(rng() % 200);
    c.dx_dz = 0.5f + (float)(rng() % 100) / 80.0f;
    const int nrec = 1 + (int)(rng() % 40);
    const int h = G / 2 + 2;  // margin along the axis
    for (int r = 0; r < nrec; r++) {
        const int z0 = c.vertical() ? h : 2, z1 = c.nzc - (c.vertical() ? h : 2), x0 = c.vertical() ? 2 : h, x1 = c.nx - (c.vertical() ? 2 : h);
        int z = z0 + (int)(rng() % (z1 - z0)), x = x0 + (int)(rng() % (x1 - x0));
        if (r > 0 && rng() % 4 == 0) {  // repeated or neighbouring channel
            z = std::min(z1 - 1, c.zr[r - 1] + (c.vertical() ? (int)(rng() % 2) : 0));
            x = std::min(x1 - 1, c.xr[r - 1] + (c.vertical() ? 0 : (int)(rng() % 2)));
        }
        c.zr.push_back(z);
        c.xr.push_back(x);
    }
    if (kind >= 2)
        for (int k = 0; k < 3 * nrec; k++) c.sens.push_back((float)((int)(rng() % 2001) - 1000) / 1000.0f);
    return c;
}

// e(p) of k_record and the sum of the magnitudes of its terms, in double
double one_cell(const Case &c, const std::vector<float> &vx, const std::vector<float> &vz, int r, int z, int x, double *mag) {
    auto VX = [&](int zz, int xx) { return (double)vx[(size_t)zz * c.nx + xx]; };
    auto VZ = [&](int zz, int xx) { return (double)vz[(size_t)zz * c.nx + xx]; };
    if (c.kind >= 2) {
        const double k = c.dx_dz, a = c.sens[3 * r], b = c.sens[3 * r + 1], s = c.sens[3 * r + 2];
        const double exx = VX(z, x) - VX(z, x - 1), ezz = (VZ(z, x) - VZ(z - 1, x)) * k;
        const double exz = 0.5 * ((VX(z + 1, x) - VX(z, x)) * k + (VZ(z, x + 1) - VZ(z, x)));
        *mag += std::fabs(a) * (std::fabs(VX(z, x)) + std::fabs(VX(z, x - 1))) + std::fabs(b) * k * (std::fabs(VZ(z, x)) + std::fabs(VZ(z - 1, x))) +
                0.5 * std::fabs(s) * ((std::fabs(VX(z + 1, x)) + std::fabs(VX(z, x))) * k + std::fabs(VZ(z, x + 1)) + std::fabs(VZ(z, x)));
        return a * exx + b * ezz + s * exz;
    }
    if (c.kind == 1) {
        *mag += std::fabs(VZ(z, x)) + std::fabs(VZ(z - 1, x));
        return VZ(z, x) - VZ(z - 1, x);
    }
    *mag += std::fabs(VX(z, x)) + std::fabs(VX(z, x - 1));
    return VX(z, x) - VX(z, x - 1);
}

double apply_taps(const GaugeTaps &t, const Case &c, const std::vector<float> &vx, const std::vector<float> &vz, int r, double *mag = nullptr) {
    double s = 0.0;
    for (int e = t.start[r]; e < t.start[r + 1]; e++) {
        const double v = (double)t.w[e] * (double)(t.field[e] ? vz : vx)[(size_t)t.z[e] * c.nx + t.x[e]];
        s += v;
        if (mag) *mag += std::fabs(v);
    }
    return s;
}

int fail(const char *what, int G, int kind) {
    printf("FAIL %s (G %d, kind %d)\n", what, G, kind);
    return 1;
}

int check_case(std::mt19937 &rng, int G, int kind) {
    const Case c = draw(rng, G, kind);
    const int nrec = (int)c.zr.size();
    const GaugeTaps t = make_gauge_taps(nrec, c.zr.data(), c.xr.data(), c.s(), c.vertical(), c.dx_dz, G);
    if ((int)t.start.size() != nrec + 1 || t.start[0] != 0 || t.start.back() != (int)t.w.size() || t.field.size() != t.w.size() ||
        t.z.size() != t.w.size() || t.x.size() != t.w.size())
        return fail("tap tables", G, kind);
    for (int r = 0; r < nrec; r++)  // ordered by (field, z, x), distinct, no zeros
        for (int e = t.start[r]; e < t.start[r + 1]; e++) {
            if (t.w[e] == 0.0f) return fail("zero tap", G, kind);
            if (e > t.start[r]) {
                const long long a = ((long long)t.field[e - 1] * c.nzc + t.z[e - 1]) * c.nx + t.x[e - 1], b = ((long long)t.field[e] * c.nzc + t.z[e]) * c.nx + t.x[e];
                if (!(a < b)) return fail("tap order", G, kind);
            }
        }
    std::vector<int> ks;
    std::vector<double> ws;
    gauge_members(G, &ks, &ws);
    // 1. taps on a random field == the definition
    std::vector<float> vx((size_t)c.nzc * c.nx), vz(vx.size());
    for (float &v : vx) v = (float)((int)(rng() % 20001) - 10000) / 3000.0f;
    for (float &v : vz) v = (float)((int)(rng() % 20001) - 10000) / 3000.0f;
    std::vector<double> Sv(nrec);
    for (int r = 0; r < nrec; r++) {
        double def = 0.0, mag = 0.0;
        for (size_t m = 0; m < ks.size(); m++) {
            double mm = 0.0;
            def += ws[m] * one_cell(c, vx, vz, r, c.zr[r] + (c.vertical() ? ks[m] : 0), c.xr[r] + (c.vertical() ? 0 : ks[m]), &mm);
            mag += ws[m] * mm;
        }
        Sv[r] = apply_taps(t, c, vx, vz, r);
        if (std::fabs(Sv[r] - def) > 1e-6 * mag + 1e-30) return fail("taps vs definition", G, kind);
    }
    // 2. straight fibres: 2 / 4 taps
    if (kind < 2)
        for (int r = 0; r < nrec; r++) {
            const int n = t.start[r + 1] - t.start[r];
            const float w = (G % 2 || G == 1) ? (float)(1.0 / G) : (float)(0.5 / G);
            if (n != ((G % 2) ? 2 : 4)) return fail("tap count", G, kind);
            for (int e = t.start[r]; e < t.start[r + 1]; e++)
                if (std::fabs(t.w[e]) != w || t.field[e] != (kind == 1 ? 1 : 0)) return fail("tap weight", G, kind);
        }
    // 3. uniform strain: the same ett for every G
    {
        const double exx = 0.375, ezz = -0.25, g1 = 0.125, g2 = 0.0625;  // vx = exx x + g1 z, vz = ezz z + g2 x (in cells; exact in float)
        std::vector<float> ux(vx.size()), uz(vz.size());
        for (int z = 0; z < c.nzc; z++)
            for (int x = 0; x < c.nx; x++) {
                ux[(size_t)z * c.nx + x] = (float)(exx * x + g1 * z);
                uz[(size_t)z * c.nx + x] = (float)(ezz * z + g2 * x);
            }
        const GaugeTaps t1 = make_gauge_taps(nrec, c.zr.data(), c.xr.data(), c.s(), c.vertical(), c.dx_dz, 1);
        for (int r = 0; r < nrec; r++) {
            double ma = 0.0, mb = 0.0;  // (the weights are rounded to float once: 1e-6 of the size of the terms)
            const double a = apply_taps(t, c, ux, uz, r, &ma), b = apply_taps(t1, c, ux, uz, r, &mb);
            if (std::fabs(a - b) > 1e-6 * (ma + mb)) return fail("uniform strain", G, kind);
        }
    }
    // 4. the plan is the exact transpose of the taps
    const int pitch = ((c.nx + 63) / 64) * 64;
    std::vector<int> tc, tf;
    const InjectPlan p = make_gauge_plan(t, c.nzc, c.nx, pitch, &tc, &tf);
    const int nseg = (c.nx + 63) / 64;
    if ((int)tc.size() != p.ntgt || (int)tf.size() != p.ntgt || (int)p.tgt_start.size() != p.ntgt + 1 || p.tgt_start.back() != (int)p.ent_rec.size())
        return fail("plan tables", G, kind);
    std::vector<double> r(nrec);
    for (double &v : r) v = (double)((int)(rng() % 20001) - 10000) / 77.0;
    double lhs = 0.0, rhs = 0.0, scale = 0.0;
    for (int q = 0; q < nrec; q++) {
        lhs += r[q] * Sv[q];
        for (int e = t.start[q]; e < t.start[q + 1]; e++)
            scale += std::fabs(r[q] * (double)t.w[e] * (double)(t.field[e] ? vz : vx)[(size_t)t.z[e] * c.nx + t.x[e]]);
    }
    for (int tg = 0; tg < p.ntgt; tg++) {
        const int z = tc[tg] / pitch, x = tc[tg] % pitch;
        if (x >= c.nx) return fail("target cell", G, kind);
        // the loop finds the target through lookup / lane mask / popcount
        const int slot = p.lookup[(size_t)z * nseg + (x >> 6)];
        if (slot < 0) return fail("lookup", G, kind);
        const InjSeg &s = p.segs[slot];
        const unsigned long long m = s.mask[tf[tg]], below = (1ull << (x & 63)) - 1ull;
        if (!((m >> (x & 63)) & 1ull) || s.base[tf[tg]] + __builtin_popcountll(m & below) != tg) return fail("lane mask", G, kind);
        double v = 0.0;
        int prev = -1;
        for (int e = p.tgt_start[tg]; e < p.tgt_start[tg + 1]; e++) {
            if (p.ent_rec[e] <= prev) return fail("entry order", G, kind);
            prev = p.ent_rec[e];
            v += (double)p.ent_w[e] * r[p.ent_rec[e]];
        }
        rhs += v * (double)(tf[tg] ? vz : vx)[(size_t)z * c.nx + x];
    }
    if (std::fabs(lhs - rhs) > 1e-12 * (scale + 1e-300)) return fail("transpose", G, kind);
    return 0;
}

Params params(int fiber, int G) {
    Params p;
    p.fiber = fiber;
    p.gauge = G;
    return p;
}

int check_bounds() {
    const int nzc = 40, nx = 50;
    for (int kind = 0; kind < 4; kind++)
        for (int G = 2; G <= 8; G++) {
            const bool vert = kind == 1 || kind == 3, dir = kind >= 2;
            const int lo = (G % 2) ? (G - 1) / 2 : G / 2;  // members reach lo cells before the channel and as many after it
            const int hi = lo;
            Survey s;
            s.nShots = 1;
            s.shots.resize(1);
            Shot &sh = s.shots[0];
            sh.present = true;
            sh.nrec = 2;
            if (dir) sh.sens.assign(6, 0.5f);
            // the lowest and highest position along the axis that keeps every member where receiver_cells allows a channel
            const int amin = (vert ? 1 : (dir ? 1 : 1)) + lo, amax = (vert ? nzc : nx) - 1 - (dir ? 1 : 0) - hi;
            const int other = vert ? nx / 2 : nzc / 2;
            auto set = [&](int a0, int a1) {
                sh.z_rec = vert ? std::vector<int>{a0, a1} : std::vector<int>{other, other};
                sh.x_rec = vert ? std::vector<int>{other, other} : std::vector<int>{a0, a1};
            };
            set(amin, amax);
            try {
                check_gauge_members(params(vert, G), s, nzc, nx);
            } catch (...) {
                return fail("members on the edge refused", G, kind);
            }
            for (int side = 0; side < 2; side++) {
                set(side ? amin : amin - 1, side ? amax + 1 : amax);
                bool threw = false;
                try {
                    check_gauge_members(params(vert, G), s, nzc, nx);
                } catch (const std::runtime_error &e) {
                    threw = std::string(e.what()).find("receiver " + std::to_string(side) + " of shot 0") != std::string::npos;
                }
                if (!threw) return fail("member outside the grid not refused", G, kind);
            }
            // the plan builder refuses taps outside the grid too
            const int zz[1] = {vert ? 0 : other}, xx[1] = {vert ? other : 0};
            const GaugeTaps t = make_gauge_taps(1, zz, xx, dir ? sh.sens.data() : nullptr, vert, 1.0f, G);
            bool threw = false;
            try {
                (void)make_gauge_plan(t, nzc, nx, 64, nullptr, nullptr);
            } catch (const std::invalid_argument &) {
                threw = true;
            }
            if (!threw) return fail("plan outside the grid", G, kind);
        }
    return 0;
}

int check_parse() {
    auto doc = [](const std::string &extra) {
        return std::string("{\"nz\": 60, \"nx\": 70, \"dz\": 5.0, \"dx\": 10.0, \"nSteps\": 10, \"dt\": 0.001, \"f0\": 10, \"nPoints_pml\": 10, "
                           "\"nPad\": 0, \"survey_fname\": \"s\", \"data_dir_name\": \"d\"") + extra + "}";
    };
    struct {
        const char *extra;
        int G;  // 0: refused
    } cases[] = {{"", 1},
                 {", \"das_gauge_length\": 10.0", 1},
                 {", \"das_gauge_length\": 30", 3},
                 {", \"das_gauge_length\": 40.005", 4},
                 {", \"das_gauge_length\": 40.02", 0},
                 {", \"das_gauge_length\": 35", 0},
                 {", \"das_gauge_length\": 0", 0},
                 {", \"das_gauge_length\": -20", 0},
                 {", \"das_gauge_length\": 4.0", 0},
                 {", \"das_gauge_length\": \"20\"", 0},
                 {", \"das_fiber\": \"vertical\", \"das_gauge_length\": 15", 3},
                 {", \"das_gauge_length\": 20, \"das_fiber\": \"vertical\"", 4},
                 {", \"das_fiber\": \"vertical\", \"das_gauge_length\": 12.5", 0}};
    for (const auto &k : cases) {
        int got = 0;
        try {
            got = parse_params(doc(k.extra)).gauge;
        } catch (const std::runtime_error &e) {
            if (std::string(e.what()).find("JSON") == std::string::npos) return fail("parse error without JSON in it", k.G, -1);
            got = 0;
        }
        if (got != k.G) {
            printf("FAIL parse %s: G %d, expected %d\n", k.extra, got, k.G);
            return 1;
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const int n = argc > 2 ? atoi(argv[2]) : 50;
    std::mt19937 rng(seed);
    int cases = 0;
    for (int G = 1; G <= 8; G++)
        for (int k = 0; k < n; k++) {
            if (check_case(rng, G, k % 4)) return 1;
            cases++;
        }
    if (check_bounds() || check_parse()) return 1;
    printf("OK %d cases\n", cases);
    return 0;
}
