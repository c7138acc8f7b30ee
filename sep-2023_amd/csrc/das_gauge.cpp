// das_gauge.cpp -- see das_gauge.hpp.  Pure host code (no HIP).
#include "das_gauge.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace sepfwi {

void gauge_members(int G, std::vector<int> *k, std::vector<double> *w) {
    k->clear();
    w->clear();
    if (G < 1) throw std::invalid_argument("gauge: G must be >= 1");
    if (G % 2) {  // midpoint rule
        for (int m = -(G - 1) / 2; m <= (G - 1) / 2; m++) {
            k->push_back(m);
            w->push_back(1.0 / G);
        }
    } else {  // trapezoid rule
        for (int m = -G / 2; m <= G / 2; m++) {
            k->push_back(m);
            w->push_back((m == -G / 2 || m == G / 2) ? 0.5 / G : 1.0 / G);
        }
    }
}

namespace {
struct Tap {
    int field, z, x;
    double w;
};
// the one-cell channel at (z, x) as taps of weight `scale` x its coefficients (k_record's expressions)
void member_taps(int z, int x, const float *s, bool vertical, double dx_dz, double scale, std::vector<Tap> *out) {
    if (s) {  // s_xx exx + s_zz ezz + s_xz exz (MOD/elasticSolver.py:266-276)
        const double a = scale * (double)s[0], b = scale * (double)s[1] * dx_dz, c = scale * 0.5 * (double)s[2];
        out->push_back({0, z, x, a});
        out->push_back({0, z, x - 1, -a});
        out->push_back({1, z, x, b});
        out->push_back({1, z - 1, x, -b});
        out->push_back({0, z + 1, x, c * dx_dz});
        out->push_back({0, z, x, -c * dx_dz});
        out->push_back({1, z, x + 1, c});
        out->push_back({1, z, x, -c});
    } else if (vertical) {  // recording_ezz
        out->push_back({1, z, x, scale});
        out->push_back({1, z - 1, x, -scale});
    } else {  // recording_exx
        out->push_back({0, z, x, scale});
        out->push_back({0, z, x - 1, -scale});
    }
}
}  // namespace

GaugeTaps make_gauge_taps(int nrec, const int *z_rec, const int *x_rec, const float *sens, bool vertical, float dx_dz, int G) {
    std::vector<int> ks;
    std::vector<double> ws;
    gauge_members(G, &ks, &ws);
    GaugeTaps t;
    t.start.assign(1, 0);
    std::vector<Tap> taps;
    for (int r = 0; r < nrec; r++) {
        taps.clear();
        for (size_t m = 0; m < ks.size(); m++) {
            const int z = z_rec[r] + (vertical ? ks[m] : 0), x = x_rec[r] + (vertical ? 0 : ks[m]);
            member_taps(z, x, sens ? sens + 3 * (size_t)r : nullptr, vertical, (double)dx_dz, ws[m], &taps);
        }
        std::sort(taps.begin(), taps.end(), [](const Tap &u, const Tap &v) {
            return u.field != v.field ? u.field < v.field : (u.z != v.z ? u.z < v.z : u.x < v.x);
        });
        for (size_t i = 0; i < taps.size();) {
            size_t j = i;
            double s = 0.0;
            for (; j < taps.size() && taps[j].field == taps[i].field && taps[j].z == taps[i].z && taps[j].x == taps[i].x; j++) s += taps[j].w;
            const float w = (float)s;
            if (w != 0.0f) {
                t.field.push_back(taps[i].field);
                t.z.push_back(taps[i].z);
                t.x.push_back(taps[i].x);
                t.w.push_back(w);
            }
            i = j;
        }
        t.start.push_back((int)t.w.size());
    }
    return t;
}

InjectPlan make_gauge_plan(const GaugeTaps &t, int nzc, int nx, int pitch, std::vector<int> *tgt_cell, std::vector<int> *tgt_field) {
    struct Add {
        int z, x, field, rec;
        float w;
    };
    InjectPlan p;
    const int nseg = (nx + 63) / 64;
    const int nrec = (int)t.start.size() - 1;
    p.lookup.assign((size_t)nzc * nseg, -1);
    std::vector<Add> adds;
    adds.reserve(t.w.size());
    for (int r = 0; r < nrec; r++)
        for (int e = t.start[r]; e < t.start[r + 1]; e++) adds.push_back({t.z[e], t.x[e], t.field[e], r, t.w[e]});
    for (const Add &a : adds)
        if (a.z < 0 || a.z >= nzc || a.x < 0 || a.x >= nx) throw std::invalid_argument("gauge plan: a channel's gauge reaches outside the grid");
    // as make_inject_plan: by row segment, field, cell; the entries of one target stay in channel order (stable)
    auto key = [&](const Add &a) { return (((long long)a.z * nseg + (a.x >> 6)) * 2 + a.field) * 64 + (a.x & 63); };
    std::stable_sort(adds.begin(), adds.end(), [&](const Add &u, const Add &v) { return key(u) < key(v); });
    if (tgt_cell) tgt_cell->clear();
    if (tgt_field) tgt_field->clear();
    long long prev = -1;
    for (const Add &a : adds) {
        const long long k = key(a);
        if (k != prev) {
            const int sidx = a.z * nseg + (a.x >> 6);
            if (p.lookup[sidx] < 0) {
                p.lookup[sidx] = (int)p.segs.size();
                p.segs.push_back(InjSeg{{0, 0}, {0, 0}, {0ull, 0ull}});
            }
            InjSeg &s = p.segs[p.lookup[sidx]];
            if (s.mask[a.field] == 0ull) s.base[a.field] = p.ntgt;
            s.mask[a.field] |= 1ull << (a.x & 63);
            p.tgt_start.push_back((int)p.ent_rec.size());
            if (tgt_cell) tgt_cell->push_back(a.z * pitch + a.x);
            if (tgt_field) tgt_field->push_back(a.field);
            p.ntgt++;
            prev = k;
        }
        p.ent_rec.push_back(a.rec);
        p.ent_w.push_back(a.w);
    }
    p.tgt_start.push_back((int)p.ent_rec.size());
    return p;
}

void check_gauge_members(const Params &par, const Survey &survey, int nzc, int nx) {
    if (par.gauge <= 1) return;
    std::vector<int> ks;
    std::vector<double> ws;
    gauge_members(par.gauge, &ks, &ws);
    const bool vertical = par.fiber != 0;
    for (size_t i = 0; i < survey.shots.size(); i++) {
        const Shot &sh = survey.shots[i];
        if (!sh.present) continue;
        const bool dir = !sh.sens.empty();
        for (int r = 0; r < sh.nrec && r < (int)sh.z_rec.size() && r < (int)sh.x_rec.size(); r++)
            for (int k : ks) {
                const int z = sh.z_rec[r] + (vertical ? k : 0), x = sh.x_rec[r] + (vertical ? 0 : k);
                // receiver_cells' bounds of a one-cell channel at the member's cell
                if (z < ((par.fiber || dir) ? 1 : 0) || z >= nzc - (dir ? 1 : 0) || x < ((par.fiber && !dir) ? 0 : 1) || x >= nx - (dir ? 1 : 0))
                    throw std::runtime_error("survey: the gauge of receiver " + std::to_string(r) + " of shot " + std::to_string(i) + " (" +
                                             std::to_string(par.gauge) + " cells) reaches outside the grid");
            }
    }
}

}  // namespace sepfwi
