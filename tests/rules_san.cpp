// Driver for the sanitizer build of the rules that contexts, batches and groups share (csrc/sots_rules.h): every check in it
// on single-fault inputs, with the code and the text it must give.  Built and run by tests/test_capi_cpu.py under
// ASan + UBSan; host code only, no HIP header.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../include/sots_hip.h"
#include "../survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd/csrc/sots_rules.h"

using namespace sots;

static int checks = 0, bad = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        ++checks;                                                \
        if (!(cond)) ++bad, printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

static bool refuses(const Fault &f, int code, const char *text) { return f.code == code && strcmp(f.text, text) == 0; }
static bool passes(const Fault &f) { return !f && f.code == SOTS_OK && f.text[0] == 0; }

static sots_config config()
{
    sots_config c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.num_parents = c.num_offspring = 16;
    c.num_dimensions = 4;
    c.audio_length_log2 = 10;
    c.synth_kind = SOTS_SYNTH_2OP;
    c.workgroup_size = 32;
    return c;
}

int main()
{
    const uint64_t ctx_limit = 1ull << 26;
    const int inv = SOTS_ERR_INVALID;
    // ---- the configuration: the table of tests/test_capi_cpu.py and tests/test_batch_cpu.py ----
    sots_config c = config();
    CHECK(passes(config_check(c, ctx_limit)) && passes(config_check(c, kNoPopulationLimit)));
    c = config(), c.struct_size = 12;
    CHECK(refuses(config_check(c, ctx_limit), inv, "sots_config.struct_size 12 != 176"));
    c = config(), c.synth_kind = 9;
    CHECK(refuses(config_check(c, ctx_limit), inv, "unknown synth_kind 9"));
    c = config(), c.num_dimensions = 6;
    CHECK(refuses(config_check(c, ctx_limit), inv, "synth_kind 0 needs numDimensions 4, got 6"));
    c = config(), c.synth_kind = SOTS_SYNTH_3OP_SERIES;
    CHECK(refuses(config_check(c, ctx_limit), inv, "synth_kind 1 needs numDimensions 6, got 4"));
    c = config(), c.audio_length_log2 = 7;
    CHECK(refuses(config_check(c, ctx_limit), inv, "audioLengthLog2 7 outside 8..15"));
    c = config(), c.audio_length_log2 = 16;
    CHECK(refuses(config_check(c, ctx_limit), inv, "audioLengthLog2 16 outside 8..15"));
    c = config(), c.audio_length_log2 = 8;
    CHECK(passes(config_check(c, ctx_limit)));
    c = config(), c.audio_length_log2 = 15;
    CHECK(passes(config_check(c, ctx_limit)));
    c = config(), c.num_parents = 0;
    CHECK(refuses(config_check(c, ctx_limit), inv, "population 16 (parents 0) not supported"));
    c = config(), c.num_parents = 1, c.num_offspring = 0, c.workgroup_size = 1;
    CHECK(refuses(config_check(c, ctx_limit), inv, "population 1 (parents 1) not supported"));
    c = config(), c.workgroup_size = 0;
    CHECK(refuses(config_check(c, ctx_limit), inv, "populationLength 32 must be a multiple of workgroupSize 0 (the recombination block)"));
    c = config(), c.workgroup_size = 24;
    CHECK(refuses(config_check(c, ctx_limit), inv, "populationLength 32 must be a multiple of workgroupSize 24 (the recombination block)"));
    c = config(), c.num_parents = 1u << 25, c.num_offspring = (1u << 25) + 32; // P > 2^26: the context's limit, not the batch's wording
    CHECK(refuses(config_check(c, ctx_limit), inv, "population 67108896 (parents 33554432) not supported"));
    CHECK(passes(config_check(c, kNoPopulationLimit)));
    c = config(), c.num_parents = 1u << 25, c.num_offspring = 1u << 25; // 2^26 exactly
    CHECK(passes(config_check(c, ctx_limit)));
    c = config(), c.num_parents = 0xFFFFFFFFu, c.num_offspring = 0xFFFFFFFFu, c.workgroup_size = 2; // the sum leaves 32 bits
    CHECK(refuses(config_check(c, ctx_limit), inv, "population 8589934590 (parents 4294967295) not supported"));
    CHECK(dims_of(SOTS_SYNTH_2OP) == 4 && dims_of(SOTS_SYNTH_3OP_SERIES) == 6 && dims_of(SOTS_SYNTH_TRIPLE_PAR) == 12 &&
          dims_of(SOTS_SYNTH_4OP_SERIES) == 8 && dims_of(4) == 0 && dims_of(0xFFFFFFFFu) == 0);
    {
        const MutateConsts mc = mutate_consts(4); // beta = sqrt(1 / 4): the two powers are square roots
        CHECK(mc.alpha == 1.4f && mc.one_over_alpha == 1.f / 1.4f && mc.beta_scale == 0.25f);
        CHECK(mc.pow_alpha_beta == powf(1.4f, 0.5f) && mc.pow_inv_alpha_beta == powf(1.f / 1.4f, 0.5f));
        CHECK(mc.root_two_over_pi == sqrtf(2.f / (float)3.14159265358979323846));
    }

    // ---- the weights ----
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    {
        std::vector<float> w(8, 1.0f), u;
        uint32_t at = 99;
        CHECK(objective_weights_check(w.data(), 7, 8, u, &at) == 1 && u.empty());
        CHECK(refuses(objective_weights_fault(w.data(), 7, 8, u), inv, "objective weights need 8 bins, got 7"));
        w[5] = -1.0f;
        CHECK(objective_weights_check(w.data(), 8, 8, u, &at) == 2 && at == 5 && u.empty());
        CHECK(refuses(objective_weights_fault(w.data(), 8, 8, u), inv, "objective weight 5 is -1: every weight must be finite and >= 0"));
        w[5] = nan;
        CHECK(objective_weights_check(w.data(), 8, 8, u, &at) == 2 && at == 5);
        w[5] = 1.0f, w[2] = inf;
        CHECK(objective_weights_check(w.data(), 8, 8, u, &at) == 2 && at == 2);
        CHECK(refuses(objective_weights_fault(w.data(), 8, 8, u), inv, "objective weight 2 is inf: every weight must be finite and >= 0"));
        w.assign(8, 0.0f);
        CHECK(objective_weights_check(w.data(), 8, 8, u, &at) == 3 && u.empty());
        CHECK(refuses(objective_weights_fault(w.data(), 8, 8, u), inv, "objective weights are all zero"));
        w[7] = 1e-38f; // one positive entry among zeros
        CHECK(objective_weights_check(w.data(), 8, 8, u, &at) == 0 && u.size() == 8 && u[0] == 0.0f && u[7] == sqrtf(1e-38f));
        for (uint32_t k = 0; k < 8; ++k) w[k] = 0.1f * (float)(k * k) + (k == 3 ? 0.0f : 1e-3f);
        u.clear();
        CHECK(passes(objective_weights_fault(w.data(), 8, 8, u)) && u.size() == 8);
        bool same = true;
        for (uint32_t k = 0; k < 8; ++k) {
            const float r = sqrtf(w[k]);
            same = same && memcmp(&r, &u[k], sizeof r) == 0; // bit for bit
        }
        CHECK(same);
        u.clear();
        CHECK(passes(objective_weights_fault(nullptr, 0, 8, u)) && u.empty()); // no weights
        CHECK(refuses(objective_weights_fault(nullptr, 8, 8, u), inv, "objective weights: a table and its length, or NULL and 0"));
        CHECK(refuses(objective_weights_fault(w.data(), 0, 8, u), inv, "objective weights: a table and its length, or NULL and 0"));
    }

    // ---- the objective and its floor ----
    CHECK(objective_floor_ok(1e-30f) && objective_floor_ok(1.0f) && objective_floor_ok(1e-6f));
    CHECK(!objective_floor_ok(std::nextafterf(1e-30f, 0.0f)) && !objective_floor_ok(std::nextafterf(1.0f, 2.0f)));
    CHECK(!objective_floor_ok(nan) && !objective_floor_ok(0.0f) && !objective_floor_ok(-1e-6f) && !objective_floor_ok(inf));
    CHECK(passes(objective_check(SOTS_OBJECTIVE_MAGNITUDE, nan))); // (the floor belongs to the log objective)
    CHECK(passes(objective_check(SOTS_OBJECTIVE_LOG_MAGNITUDE, 1e-30f)) && passes(objective_check(SOTS_OBJECTIVE_LOG_MAGNITUDE, 1.0f)));
    CHECK(refuses(objective_check(SOTS_OBJECTIVE_LOG_MAGNITUDE, 2.0f), inv, "log-magnitude floor 2 outside 1e-30 .. 1"));
    CHECK(refuses(objective_check(SOTS_OBJECTIVE_LOG_MAGNITUDE, nan), inv, "log-magnitude floor nan outside 1e-30 .. 1"));
    CHECK(objective_check(SOTS_OBJECTIVE_LOG_MAGNITUDE, std::nextafterf(1e-30f, 0.0f)).code == inv);
    CHECK(refuses(objective_check(7, 1e-6f), inv, "unknown objective 7 (0 = magnitude, 1 = log magnitude)"));

    // ---- the run record's arguments: a context (no chunk count), a batch ----
    {
        uint32_t f = 0;
        CHECK(passes(track_args_check(&f, 0, 0, 0)) && f == 0);
        f = SOTS_TRACK_BEST_EVER;
        CHECK(passes(track_args_check(&f, 0, 0, 64)) && f == SOTS_TRACK_BEST_EVER);
        f = SOTS_TRACK_HISTORY;
        CHECK(passes(track_args_check(&f, 1, 1, 0)) && f == (SOTS_TRACK_HISTORY | SOTS_TRACK_BEST_EVER)); // HISTORY implies BEST_EVER
        f = 8;
        CHECK(refuses(track_args_check(&f, 1, 1, 0), inv, "unknown track flags 8"));
        f = SOTS_TRACK_HISTORY;
        CHECK(refuses(track_args_check(&f, 0, 4, 0), inv, "history needs history_every >= 1 and history_capacity >= 1 (got 0, 4)"));
        f = SOTS_TRACK_HISTORY;
        CHECK(refuses(track_args_check(&f, 2, 0, 8), inv, "history needs history_every >= 1 and history_capacity >= 1 (got 2, 0)"));
        f = SOTS_TRACK_HISTORY;
        CHECK(passes(track_args_check(&f, 1, 1u << 24, 0)) && passes(track_args_check(&f, 1, 1u << 18, 64)));
        CHECK(refuses(track_args_check(&f, 1, (1u << 24) + 1, 0), inv, "history_capacity 16777217 exceeds 16777216 records"));
        CHECK(refuses(track_args_check(&f, 1, (1u << 18) + 1, 64), inv, "history_capacity 262145 x max_chunks 64 exceeds 16777216 records"));
        CHECK(refuses(track_args_check(&f, 1, 0xFFFFFFFFu, 0xFFFFFFFFu), inv, "history_capacity 4294967295 x max_chunks 4294967295 exceeds 16777216 records"));
    }
    {
        sots_stop_rule r;
        memset(&r, 0, sizeof r);
        r.struct_size = sizeof r, r.check_interval = 25;
        CHECK(stop_rule_check(&r) == SOTS_OK && stop_rule_check(nullptr) == inv);
        r.check_interval = 0;
        CHECK(stop_rule_check(&r) == inv);
        r.check_interval = 1, r.struct_size = 4;
        CHECK(stop_rule_check(&r) == inv);
    }

    // ---- the rows: numParents below one block, one block, a multiple of the block, not a multiple ----
    CHECK(breeding_rows(16, 32) == 32 && selected_rows(16, 32) == 32); // one block is read whatever the parents
    CHECK(breeding_rows(1, 32) == 32 && selected_rows(1, 32) == 32);
    CHECK(breeding_rows(32, 32) == 32 && selected_rows(32, 32) == 32);
    CHECK(breeding_rows(96, 32) == 96 && selected_rows(96, 32) == 96);
    CHECK(breeding_rows(100, 32) == 96 && selected_rows(100, 32) == 100); // rows 96..99: placed, never read
    CHECK(breeding_rows(33, 32) == 32 && selected_rows(33, 32) == 33);
    CHECK(breeding_rows(7, 1) == 7 && selected_rows(7, 1) == 7);
    CHECK(breeding_rows(7, 0) == 7 && selected_rows(7, 0) == 7); // (no block: rows one by one, not a division by zero)
    CHECK(breeding_rows(0xFFFFFFFFu, 32) == 0xFFFFFFE0u && selected_rows(0xFFFFFFFFu, 32) == 0xFFFFFFFFu);

    // ---- population byte counts ----
    {
        float x = 0;
        CHECK(passes(population_bytes_check(32, 4, &x, 512, &x, 512, &x, 128)));
        CHECK(passes(population_bytes_check(32, 4, nullptr, 7, nullptr, 7, nullptr, 7))); // an array not passed is not counted
        CHECK(refuses(population_bytes_check(32, 4, &x, 511, nullptr, 0, nullptr, 0), SOTS_ERR_SIZE,
                      "population byte counts must be 512 (values, steps) and 128 (fitness)"));
        CHECK(population_bytes_check(32, 4, nullptr, 0, &x, 516, nullptr, 0).code == SOTS_ERR_SIZE);
        CHECK(population_bytes_check(32, 4, nullptr, 0, nullptr, 0, &x, 512).code == SOTS_ERR_SIZE);
        CHECK(passes(population_bytes_check(1u << 26, 12, &x, (size_t)12 << 28, nullptr, 0, &x, (size_t)1 << 28))); // past 2^31 bytes
    }
    printf("shared rules: %d checks, %d failures\n", checks, bad);
    return bad ? 1 : 0;
}
