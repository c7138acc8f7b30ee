// geophone.cpp -- see geophone.hpp.  Pure host code (no HIP).
#include "geophone.hpp"

namespace sepfwi {

int geo_blocks(const Params &par, int block_of_comp[4]) {
    int n = 0;
    for (int c = 0; c < 4; c++) block_of_comp[c] = -1;
    for (int comp : kGeoOrder)
        if (par.weight(comp) > 0.0f) block_of_comp[comp] = n++;
    return n;
}

GaugeTaps make_geophone_taps(int nrec, const int *z_rec, const int *x_rec, const float *sens, bool vertical, float dx_dz, int G, bool with_ett,
                             bool with_vx, bool with_vz) {
    GaugeTaps t;
    if (with_ett)
        t = make_gauge_taps(nrec, z_rec, x_rec, sens, vertical, dx_dz, G);
    else
        t.start.assign(1, 0);
    for (int field = 0; field < 2; field++) {  // vx geophones, then vz geophones: one tap of weight 1 at the channel's own cell
        if (!(field ? with_vz : with_vx)) continue;
        for (int r = 0; r < nrec; r++) {
            t.field.push_back(field);
            t.z.push_back(z_rec[r]);
            t.x.push_back(x_rec[r]);
            t.w.push_back(1.0f);
            t.start.push_back((int)t.w.size());
        }
    }
    return t;
}

}  // namespace sepfwi
