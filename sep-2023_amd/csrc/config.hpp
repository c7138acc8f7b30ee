// config.hpp -- parameter / survey description of one propagation setup.
// Same JSON schema as the reference (writer: fwi_utils.py:46-124; readers it replaces:
// Src/Parameter.cpp:17-178 and Src/Src_Rec.cu:20-281).
#pragma once
#include <string>
#include <vector>

namespace sepfwi {

// The misfit kind of a parameter file, and per kind the facts that the parser and the session branch on.  A new kind is a new enumerator,
// a new row and a new case in the switches over Params::misfit (none has a default: the compiler names the ones that miss it).
enum class Misfit { L2, Cross, Envelope, W2, Robust };
struct MisfitTraits {
    const char *key;        // the JSON key that selects the kind (nullptr: L2, the absence of the others)
    bool gauss_newton;      // a Gauss-Newton product exists: born's hv_*, the exact product, data_gn (the others are no least squares of the data)
    bool at_background;     // ... and it linearises at the shot's BACKGROUND gather, which those calls record or take (syn)
    bool needs_obs;         // ... and it needs the conditioned observed gather (the IRLS weight)
    bool exact_adjoint;     // adjoint_exact serves the kind's gradient
    bool trace_weights;     // the residual takes the survey's trace weights and src_weight explicitly (under if_win)
    bool with_src_update;   // parse_params accepts if_src_update beside the key (Cross: Session's constructor refuses the pair, after the survey is read)
};
constexpr MisfitTraits kMisfitTraits[] = {
    //                         key             gn     at_bg  obs    exact  trace_w  src_update
    /* L2       */ {nullptr,               true,  false, false, true,  false, true},
    /* Cross    */ {"if_cross_misfit",     false, false, false, false, true,  true},
    /* Envelope */ {"if_envelope_misfit",  true,  true,  false, true,  false, false},
    /* W2       */ {"if_w2_misfit",        false, false, false, true,  true,  false},
    /* Robust   */ {"robust_misfit",       true,  true,  true,  true,  false, false},
};
constexpr int kMisfitKinds = (int)Misfit::Robust + 1;
static_assert(sizeof(kMisfitTraits) / sizeof(kMisfitTraits[0]) == kMisfitKinds, "one row of kMisfitTraits per Misfit kind, in the enum's order");
inline const MisfitTraits &traits(Misfit m) { return kMisfitTraits[(int)m]; }

struct Params {
    int nz = 0, nx = 0;  // padded grid sizes
    float dz = 0, dx = 0, dt = 0, f0 = 0;
    int nSteps = 0, nPml = 0, nPad = 0;
    std::string survey_fname, data_dir_name, scratch_dir_name;
    // optional key "obs_pack_fname" (SURVEY.md 8f-2): ONE packed file of the survey's observed axial-strain gathers (layout:
    // sepfwi/utils.py pack_observed) instead of the reference's four files per shot (libCUFD.cu:216-223)
    std::string obs_pack_fname;
    // optional key "obs_cache_mb": HBM budget [MB] of the session's observed-data store; the least recently used gathers beyond it
    // wait in pinned host memory (obs_store.hpp).  0 / absent: no budget (option "obs_cache_mb" of sepfwi_set_option applies).
    int obs_cache_mb = 0;
    // data-conditioning keys (dormant in the reference's driver, libCUFD.cu:353-457; live here, csrc/conditioning.hip).  if_src_update is a
    // stage of the chain (the matching filter), not a misfit kind; kMisfitTraits says which kinds it may accompany.
    bool if_win = false, if_src_update = false, has_filter = false;
    // the file's misfit kind, from the keys "if_cross_misfit" / "if_envelope_misfit" / "if_w2_misfit" / "robust_misfit" ("huber" | "cauchy")
    // (live conditioning keys like those above; at most one may be set).  What the kinds compute: include/sepfwi.h, sepfwi_cufd, and
    // conditioning.hpp, w2_misfit.hpp, robust_misfit.hpp; what each serves and is refused with: kMisfitTraits, nowhere else.  Their numbers:
    // w2_beta in (0, 16]; robust_delta REQUIRED with robust_misfit (finite, above 0; no default: it depends on the data's noise),
    // robust_quantile in (0, 1]; robust_delta or robust_quantile without robust_misfit is refused.
    Misfit misfit = Misfit::L2;
    double w2_beta = 3.0;
    int robust_kind = 0;  // RobustKind (robust_misfit.hpp): 1 huber, 2 cauchy; 0 unless misfit is Robust
    double robust_delta = 0.0, robust_quantile = 0.9;
    // optional keys "fk_slowness" [p1, p2, p3, p4] (s/m) / "fk_mode" ("pass" | "reject", default "pass") (no counterpart in the reference;
    // conditioning.hpp, fk_filter): the apparent-slowness fan filter across a shot's channels, the third stage of the chain,
    // C = FK . band-pass . window.  Four finite numbers p1 < p2 <= p3 < p4 (negative ones allowed: p > 0 is an event that arrives later at
    // higher channel indices); fk_mode without fk_slowness is refused.  A live conditioning key like those above.  The channel spacing
    // comes from the survey: every shot's channels must lie on one straight, equally spaced line (host_checks.hpp: fk_channel_spacing;
    // refused at session creation otherwise).
    bool has_fk = false, fk_reject = false;
    double fk_slowness[4] = {0, 0, 0, 0};
    // optional key "conditioning": "live" (default) -- the keys above switch their stage on; "reference" -- they are parsed
    // and validated like the reference does and then IGNORED like its driver does (every call site commented out,
    // libCUFD.cu:353-457): results are those of a file without them.  if_win_key keeps what the file said, because the survey
    // file must carry win_start / win_end whenever if_win is set, used or not (Src_Rec.cu:144-174).
    bool conditioning_reference = false, if_win_key = false;
    float filter[4] = {0, 0, 0, 0};  // band-pass corner frequencies [Hz]   (Parameter.cpp:147-159)
    // optional key "das_fiber": "horizontal" (default; recording_exx / res_injection_exx, libCUFD.cu:325,607) or
    // "vertical" (recording_ezz / res_injection_ezz, utilities.cu:620-641 -- in the reference a source edit)
    int fiber = 0;
    // optional key "das_gauge_length" [m] (das_gauge.hpp): every channel records the mean axial strain over G = round(L / dx) cells
    // along a horizontal fibre, round(L / dz) along a vertical one.  1 (absent): the one-cell channel.
    int gauge = 1;
    // optional keys "misfit_w_ett" / "misfit_w_vx" / "misfit_w_vz" (geophone.hpp): weights of the axial-strain, vx and vz residuals in
    // misfit and adjoint source.  Absent or (1, 0, 0): the axial-strain misfit of the reference's driver, on the path it always took.
    float w_ett = 1.0f, w_vx = 0.0f, w_vz = 0.0f;
    bool joint() const { return !(w_ett == 1.0f && w_vx == 0.0f && w_vz == 0.0f); }  // the joint path (geophone.hip) serves the call
    float weight(int comp) const { return comp == 1 ? w_vx : (comp == 2 ? w_vz : (comp == 3 ? w_ett : 0.0f)); }  // comp: 1 vx, 2 vz, 3 ett
    // The first live conditioning key in the order if_win, filter, if_cross_misfit, if_src_update, if_envelope_misfit, if_w2_misfit,
    // robust_misfit, fk_slowness, or nullptr: a file without one has C = 1 and no conditioner.  Joint weights are refused with any.
    const char *first_live_key() const;
};

struct Shot {
    int z_src = 0, x_src = 0;  // already shifted by +nPml (Src_Rec.cu:87-92)
    int nrec = 0;
    std::vector<int> z_rec, x_rec;  // shifted by +nPml (Src_Rec.cu:107-115)
    double src_rxz = 1.0;           // RSXXZZ default, Src_Rec.cu:259-264
    // optional key "das_sensitivity" (nrec x 6, the Numba solver's layout: column 0 weighs exx, 3 ezz, 1 exz,
    // MOD/elasticSolver.py:152-153,276): per-channel directional sensitivities, stored as (s_xx, s_zz, s_xz) triples.
    // Empty: straight fibre along x or z (para key "das_fiber").
    std::vector<float> sens;
    // with if_win: per-channel time windows [s] and trace weights, shot weight (Src_Rec.cu:144-200); weights default to 1
    std::vector<float> win_start, win_end, weights;
    float src_weight = 1.0f;
    bool present = false;
};

struct Survey {
    int nShots = 0;
    std::vector<Shot> shots;  // indexed by shot id ("shot%d" keys)
    int max_nrec = 0;
};

// Read the first line of a file (the reference only reads one line: Parameter.cpp:29, Src_Rec.cu:32).
// Throws std::runtime_error("EIO: ...") if the file cannot be opened.
std::string read_first_line(const std::string &fname);

// Parse; throw std::runtime_error on malformed input.
Params parse_params(const std::string &json_text);
Survey parse_survey(const std::string &json_text, int nPml, bool if_win = false);

// C-PML 1-D profiles (replaces cpmlInit, Src/utilities.cu:243-359).
void cpml_profiles(float *K, float *a, float *b, float *K_half, float *a_half, float *b_half, int N, int nPml,
                   float dh, float f0, float dt);

// sin^2 / cos^2 end taper of a trace (replaces the 5-argument cuda_window, Src/utilities.cu:844-884).
// Returns false (trace untouched) in the reference's "Window error 2" case.
bool stf_taper(float *trace, int nt, float dt, float ratio);

// Contiguous split of `group_size` shots over `ngpu` devices (Src/Torch_Fwi.cpp:59-60,78-80):
// starts[i] = (int) float32 linspace(0, group_size, ngpu+1)[i].
void shot_split(int group_size, int ngpu, int *starts);

}  // namespace sepfwi
