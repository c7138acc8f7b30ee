// CPU-only check of the parameter key "if_envelope_misfit" in the host-side parser of libsepfwi (csrc/config.cpp): built with
// -fsanitize=address,undefined by tests/test_envelope_config.py.  The key parses, "conditioning": "reference" ignores it like the
// other four conditioning keys, and the three combinations without a meaning are refused with std::invalid_argument -- the class that
// the C ABI reports as SEPFWI_EINVAL (csrc/capi.cpp; a std::runtime_error that names JSON would be SEPFWI_EJSON) -- in a message that
// names both keys.
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../sep-2023_amd/csrc/config.hpp"

using namespace sepfwi;

static const char *BASE =
    "{\"nz\": 96, \"nx\": 80, \"dz\": 10.0, \"dx\": 10.0, \"nSteps\": 100, \"dt\": 0.001, \"f0\": 10.0, \"nPoints_pml\": 10, "
    "\"nPad\": 12, \"survey_fname\": \"s.json\", \"data_dir_name\": \"D\"";

static std::string doc(const std::string &more) { return std::string(BASE) + more + "}"; }

static int failures = 0;
static void fail(const char *what) {
    printf("FAIL: %s\n", what);
    failures++;
}

// -> 0 accepted, 1 std::invalid_argument naming both keys, 2 std::invalid_argument with another message, 3 any other exception
static int refusal(const std::string &more, const char *key_a, const char *key_b) {
    try {
        (void)parse_params(doc(more));
    } catch (const std::invalid_argument &e) {
        const std::string w = e.what();
        return (w.find(key_a) != std::string::npos && w.find(key_b) != std::string::npos) ? 1 : 2;
    } catch (const std::exception &) {
        return 3;
    }
    return 0;
}

int main() {
    // the key parsed; absent or false: off
    if (parse_params(doc("")).misfit == Misfit::Envelope) fail("absent key reads as set");
    if (parse_params(doc(", \"if_envelope_misfit\": false")).misfit == Misfit::Envelope) fail("false reads as set");
    {
        const Params p = parse_params(doc(", \"if_envelope_misfit\": true"));
        if (p.misfit != Misfit::Envelope || p.if_win || p.has_filter || p.misfit == Misfit::Cross || p.if_src_update || p.joint()) fail("the key alone mis-parsed");
    }
    {   // it composes with if_win and filter
        const Params p = parse_params(doc(", \"if_envelope_misfit\": true, \"if_win\": true, \"filter\": [1.0, 2.0, 8.0, 10.0]"));
        if (p.misfit != Misfit::Envelope || !p.if_win || !p.has_filter || p.filter[2] != 8.0f) fail("the key with if_win and filter mis-parsed");
    }
    {   // a value that is no boolean: the reader's own error (not std::invalid_argument)
        bool threw = false;
        try { (void)parse_params(doc(", \"if_envelope_misfit\": 3")); } catch (const std::invalid_argument &) {} catch (const std::exception &) { threw = true; }
        if (!threw) fail("a numeric value of the key accepted or misreported");
    }
    {   // reference mode: parsed, then ignored like the other four -- also in the combinations that a live file refuses
        const Params p = parse_params(doc(", \"if_envelope_misfit\": true, \"if_cross_misfit\": true, \"if_win\": true, \"conditioning\": \"reference\""));
        if (!p.conditioning_reference || p.misfit == Misfit::Envelope || p.misfit == Misfit::Cross || p.if_win || !p.if_win_key) fail("reference mode does not ignore the key");
        const Params q = parse_params(doc(", \"if_envelope_misfit\": true, \"misfit_w_vx\": 0.5, \"conditioning\": \"reference\""));
        if (q.misfit == Misfit::Envelope || !q.joint()) fail("reference mode with joint weights mis-parsed");
        const Params r = parse_params(doc(", \"if_envelope_misfit\": true, \"conditioning\": \"live\""));
        if (r.misfit != Misfit::Envelope) fail("conditioning = live drops the key");
    }
    // the refused pairs, each naming both keys, as std::invalid_argument
    if (refusal(", \"if_envelope_misfit\": true, \"if_cross_misfit\": true", "if_envelope_misfit", "if_cross_misfit") != 1) fail("if_cross_misfit pair");
    if (refusal(", \"if_envelope_misfit\": true, \"if_src_update\": true", "if_envelope_misfit", "if_src_update") != 1) fail("if_src_update pair");
    if (refusal(", \"if_envelope_misfit\": true, \"if_win\": true, \"filter\": [1.0, 2.0, 8.0, 10.0], \"if_src_update\": true", "if_envelope_misfit", "if_src_update") != 1)
        fail("if_src_update pair on top of if_win and filter");
    // joint weights other than (1, 0, 0) with the key as the only live conditioning key
    if (refusal(", \"if_envelope_misfit\": true, \"misfit_w_vx\": 0.5", "misfit_w_vx", "if_envelope_misfit") != 1) fail("joint weights (vx)");
    if (refusal(", \"if_envelope_misfit\": true, \"misfit_w_vz\": 2.0", "misfit_w_vz", "if_envelope_misfit") != 1) fail("joint weights (vz)");
    if (refusal(", \"if_envelope_misfit\": true, \"misfit_w_ett\": 0.5", "misfit_w_ett", "if_envelope_misfit") != 1) fail("joint weights (ett alone, not 1)");
    // ... and what the rule said before stays word for word: the first live key of the old order is the one named
    if (refusal(", \"if_envelope_misfit\": true, \"if_win\": true, \"misfit_w_vx\": 0.5", "misfit_w_vx", "if_win") != 1) fail("joint weights with if_win");
    if (refusal(", \"if_cross_misfit\": true, \"misfit_w_vx\": 0.5", "misfit_w_vx", "if_cross_misfit") != 1) fail("joint weights with if_cross_misfit");
    // explicit default weights are no joint misfit: accepted
    if (refusal(", \"if_envelope_misfit\": true, \"misfit_w_ett\": 1.0, \"misfit_w_vx\": 0.0", "", "") != 0) fail("default weights refused");
    // without the key the two old keys are still accepted by the parser (their own combination is the session's business)
    if (refusal(", \"if_cross_misfit\": true", "", "") != 0 || refusal(", \"if_src_update\": true", "", "") != 0) fail("a file without the key refused");
    if (failures) return 1;
    printf("OK\n");
    return 0;
}
