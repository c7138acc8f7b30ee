// CPU-only check of which combinations of the misfit-kind keys and "if_src_update" the host-side parser of libsepfwi (csrc/config.cpp)
// accepts, and of the exact message of every refusal: built with -fsanitize=address,undefined by tests/test_misfit_keys.py.
//
// EXPECT holds the outcome of each of the 32 subsets of {if_cross_misfit, if_envelope_misfit, if_w2_misfit, robust_misfit, if_src_update}
// (bit k of the index: key k of that list; nullptr: accepted).  The literals were recorded from the parser as it stood BEFORE the misfit
// kind became one enum (three hand-written ladders, one per key), by a program that fed it these same 32 documents and printed what() --
// not from the code this check is built against.  The second half walks the 256 subsets of the eight live conditioning keys under joint
// weights, whose outcome the 32 literals and the key order of the joint-weights refusal determine.
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../sep-2023_amd/csrc/config.hpp"

using namespace sepfwi;

static const char *BASE =
    "{\"nz\": 96, \"nx\": 80, \"dz\": 10.0, \"dx\": 10.0, \"nSteps\": 100, \"dt\": 0.001, \"f0\": 10.0, \"nPoints_pml\": 10, "
    "\"nPad\": 12, \"survey_fname\": \"s.json\", \"data_dir_name\": \"D\"";

// the five keys of EXPECT's index, bit 0 first
static const char *FIVE[5] = {", \"if_cross_misfit\": true", ", \"if_envelope_misfit\": true", ", \"if_w2_misfit\": true",
                              ", \"robust_misfit\": \"huber\", \"robust_delta\": 1.5", ", \"if_src_update\": true"};

static const char *EXPECT[32] = {
    nullptr,                                                                                // 0
    nullptr,                                                                                // 1
    nullptr,                                                                                // 2
    "parameter file: if_envelope_misfit together with if_cross_misfit is not supported",    // 3
    nullptr,                                                                                // 4
    "parameter file: if_w2_misfit together with if_cross_misfit is not supported",          // 5
    "parameter file: if_w2_misfit together with if_envelope_misfit is not supported",       // 6
    "parameter file: if_envelope_misfit together with if_cross_misfit is not supported",    // 7
    nullptr,                                                                                // 8
    "parameter file: robust_misfit together with if_cross_misfit is not supported",         // 9
    "parameter file: robust_misfit together with if_envelope_misfit is not supported",      // 10
    "parameter file: if_envelope_misfit together with if_cross_misfit is not supported",    // 11
    "parameter file: robust_misfit together with if_w2_misfit is not supported",            // 12
    "parameter file: if_w2_misfit together with if_cross_misfit is not supported",          // 13
    "parameter file: if_w2_misfit together with if_envelope_misfit is not supported",       // 14
    "parameter file: if_envelope_misfit together with if_cross_misfit is not supported",    // 15
    nullptr,                                                                                // 16
    nullptr,                                                                                // 17
    "parameter file: if_envelope_misfit together with if_src_update is not supported",      // 18
    "parameter file: if_envelope_misfit together with if_cross_misfit is not supported",    // 19
    "parameter file: if_w2_misfit together with if_src_update is not supported",            // 20
    "parameter file: if_w2_misfit together with if_cross_misfit is not supported",          // 21
    "parameter file: if_envelope_misfit together with if_src_update is not supported",      // 22
    "parameter file: if_envelope_misfit together with if_cross_misfit is not supported",    // 23
    "parameter file: robust_misfit together with if_src_update is not supported",           // 24
    "parameter file: robust_misfit together with if_cross_misfit is not supported",         // 25
    "parameter file: if_envelope_misfit together with if_src_update is not supported",      // 26
    "parameter file: if_envelope_misfit together with if_cross_misfit is not supported",    // 27
    "parameter file: if_w2_misfit together with if_src_update is not supported",            // 28
    "parameter file: if_w2_misfit together with if_cross_misfit is not supported",          // 29
    "parameter file: if_envelope_misfit together with if_src_update is not supported",      // 30
    "parameter file: if_envelope_misfit together with if_cross_misfit is not supported",    // 31
};

// the eight live conditioning keys in the order in which the joint-weights refusal names the first one set; five: its bit in EXPECT's
// index, or -1
static const struct {
    const char *name, *json;
    int five;
} LIVE[8] = {{"if_win", ", \"if_win\": true", -1},
             {"filter", ", \"filter\": [1.0, 2.0, 8.0, 10.0]", -1},
             {"if_cross_misfit", FIVE[0], 0},
             {"if_src_update", FIVE[4], 4},
             {"if_envelope_misfit", FIVE[1], 1},
             {"if_w2_misfit", FIVE[2], 2},
             {"robust_misfit", FIVE[3], 3},
             {"fk_slowness", ", \"fk_slowness\": [-0.002, -0.001, 0.001, 0.002]", -1}};

static int failures = 0;

// parse BASE + more + "}" and compare the outcome with `expect` (nullptr: accepted; else the what() of a std::invalid_argument)
static void check(const std::string &label, const std::string &more, const std::string *expect) {
    std::string got = "accepted";
    try {
        (void)parse_params(std::string(BASE) + more + "}");
    } catch (const std::invalid_argument &e) {
        got = std::string("invalid_argument: ") + e.what();
    } catch (const std::exception &e) {
        got = std::string("another exception: ") + e.what();
    }
    const std::string want = expect ? "invalid_argument: " + *expect : "accepted";
    if (got != want) {
        printf("FAIL: %s\n  expected  %s\n  got       %s\n", label.c_str(), want.c_str(), got.c_str());
        failures++;
    }
}

int main() {
    for (int s = 0; s < 32; s++) {
        std::string more;
        for (int k = 0; k < 5; k++)
            if (s >> k & 1) more += FIVE[k];
        const std::string want = EXPECT[s] ? EXPECT[s] : "";
        check("subset " + std::to_string(s) + " of the five keys", more, EXPECT[s] ? &want : nullptr);
    }
    for (int s = 0; s < 256; s++) {
        std::string more = ", \"misfit_w_vx\": 0.5";
        int five = 0;
        const char *first = nullptr;
        for (int k = 0; k < 8; k++) {
            if (!(s >> k & 1)) continue;
            more += LIVE[k].json;
            if (LIVE[k].five >= 0) five |= 1 << LIVE[k].five;
            if (!first) first = LIVE[k].name;
        }
        std::string want;
        if (EXPECT[five])
            want = EXPECT[five];
        else if (first)
            want = std::string("parameter file: misfit_w_vx together with the live conditioning key ") + first +
                   " is not supported (the conditioning chain acts on axial-strain gathers weighted 1)";
        check("subset " + std::to_string(s) + " of the eight live keys under misfit_w_vx", more, (EXPECT[five] || first) ? &want : nullptr);
    }
    if (failures) return 1;
    printf("OK\n");
    return 0;
}
