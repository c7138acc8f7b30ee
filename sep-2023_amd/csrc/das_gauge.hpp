// das_gauge.hpp -- DAS gauge length (parameter key "das_gauge_length"): every channel records the mean axial strain over a gauge of
// G cells along the fibre instead of the strain of its own cell.
//
// With e(p) the one-cell channel value at cell p (k_record: vx(z,x) - vx(z,x-1) for a horizontal fibre, vz(z,x) - vz(z-1,x) for a
// vertical one, s_xx exx + s_zz ezz + s_xz exz for a directional channel) and a the fibre axis (x horizontal, z vertical):
//   ett(p) = sum_k w_k e(p + k a)
//     G odd : k = -(G-1)/2 ... (G-1)/2,  w_k = 1/G
//     G even: k = -G/2 ... G/2,          w_k = 1/G inside, 1/(2G) at both ends
// -- the gauge integral divided by the gauge length of dasResponse.py over the grid's one-cell strains (midpoint rule for odd G,
// trapezoid rule for even G), centred on the channel's own strain point.  sum w_k = 1.  The sum is linear in vx / vz, so a channel is
// a short list of TAPS (field, cell, weight): straight fibres telescope to 2 (odd G) or 4 (even G) taps.  Its adjoint source is the
// exact transpose, an InjectPlan (inject_plan.hpp) built from the taps.
//
// Pure host code (no HIP): unit-tested on the CPU under the sanitizers (tests/native/das_gauge_check.cpp).  The device side
// (k_record_gauge, k_inject_gauge and their batched twins) lives in das_gauge.hip; the session only takes it for G > 1.
#pragma once
#include <vector>

#include "config.hpp"
#include "inject_plan.hpp"

namespace sepfwi {

// Members k and weights w_k of a gauge of G >= 1 cells (G == 1: the channel itself, weight 1).
void gauge_members(int G, std::vector<int> *k, std::vector<double> *w);

// One shot's channels as taps, CSR: channel r owns entries start[r] .. start[r + 1]; field 0 vx, 1 vz.  Entries of one channel that
// hit the same (field, cell) are summed in double and rounded once, zeros are dropped, and the entries are ordered by (field, z, x).
struct GaugeTaps {
    std::vector<int> start;  // [nrec + 1]
    std::vector<int> field, z, x;
    std::vector<float> w;
};

// z_rec / x_rec: the channels in padded grid coordinates; sens: null or nrec x 3 (s_xx, s_zz, s_xz); vertical: the fibre (and the
// gauge) runs along z; dx_dz = dx / dz as the kernels form it (g.dx * g.rdz).
GaugeTaps make_gauge_taps(int nrec, const int *z_rec, const int *x_rec, const float *sens, bool vertical, float dx_dz, int G);

// The adjoint of the taps: targets sorted as make_inject_plan sorts them, entries of a target in channel order.  tgt_cell / tgt_field
// (may be null): per target its flat index z * pitch + x and its field, for the injection kernel of the per-step schedules.
// Throws std::invalid_argument when a tap lies outside the nzc x nx grid.
InjectPlan make_gauge_plan(const GaugeTaps &t, int nzc, int nx, int pitch, std::vector<int> *tgt_cell, std::vector<int> *tgt_field);

// Every member of every channel of every present shot where receiver_cells (host_checks.hpp) allows a one-cell channel.  Throws
// std::runtime_error naming the shot and the channel.  Nothing to check for G == 1.
void check_gauge_members(const Params &par, const Survey &survey, int nzc, int nx);

// Device-side description of one shot's gauge channels for the batched schedule (the side table of ShotDev, indexed alike).  A shot
// without gauge channels has nrec == ntgt == 0.  Its fields, seismograms, adjoint fields and residual are those of its ShotDev entry,
// whose own nrec is 0 for a gauge shot so that the generic receiver kernels skip it.  A joint DAS + geophone misfit (geophone.hpp)
// injects every shot through the plan part of its entry (nrec stays 0 there unless the shot has gauge channels).
struct GaugeShotDev {
    int nrec, ntgt, comps;
    int nres;                                              // row length of the adjoint-source array: nrec, or the concatenated length of a joint misfit (geophone.hpp)
    const int *rec;                                        // [nrec] the channels' own cells (pr / vx / vz)
    const int *tap_start, *tap_cell, *tap_field;           // taps, CSR over channels
    const float *tap_w;
    const int *tgt_start, *tgt_cell, *tgt_field, *ent_rec;  // adjoint plan: targets and their (channel, weight) entries
    const float *ent_w;
};

}  // namespace sepfwi
