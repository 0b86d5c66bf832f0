// graph_feedback_genes_san.cpp -- the rules of feedback indices as genes (csrc/sots_rules.h: voice_feedback_genes_check
// through config_check, graph_dims, feedback_gene_column, effective_feedback, the mask in voice_feedback_check /
// voice_feedback_set and in the two continuous renderers' checks, voice_feedback_genes_get_check): every refusal with the
// code and the text it must give, what passes, and the numbers that follow from a mask.  Built and run by
// tests/test_graph_feedback_genes_cpu.py under ASan + UBSan; host code only, no HIP header.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../include/sots_hip.h"
#include "../survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd/csrc/sots_rules.h"

using namespace sots;

static int checks = 0, bad = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        ++checks;                                                \
        if (!(cond)) ++bad, printf("line %d: %s\n", __LINE__, #cond); \
    } while (0)

static bool refuses(const Fault &f, int code, const char *text)
{
    const bool ok = f.code == code && strcmp(f.text, text) == 0;
    if (!ok) printf("  got %d \"%s\"\n", f.code, f.text);
    return ok;
}
static bool passes(const Fault &f)
{
    if (f) printf("  got %d \"%s\"\n", f.code, f.text);
    return !f && f.code == SOTS_OK && f.text[0] == 0;
}
static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

// a chain 0 -> 1 -> ... -> ops-1, the last one heard
static sots_voice_graph chain(uint32_t ops)
{
    sots_voice_graph g{};
    g.struct_size = sizeof g;
    g.num_operators = ops;
    g.carriers = 1u << (ops - 1u);
    for (uint32_t j = 1; j < ops; ++j) g.modulators[j] = 1u << (j - 1u);
    return g;
}
// 32 + 32 rows, block 32, N = 256; d genes, the first 2 ops of them frequencies and levels, the rest in [0, 2]
static sots_config config(uint32_t ops, uint32_t d)
{
    sots_config c{};
    c.struct_size = sizeof c;
    c.num_parents = c.num_offspring = c.workgroup_size = 32;
    c.num_dimensions = d;
    c.audio_length_log2 = 8;
    c.synth_kind = SOTS_SYNTH_GRAPH;
    for (uint32_t g = 0; g < SOTS_MAX_DIMS; ++g) c.param_max[g] = g < 2u * ops ? (g % 2u ? 8.0f : 3520.0f) : 2.0f;
    return c;
}

int main()
{
    const int inv = SOTS_ERR_INVALID, state = SOTS_ERR_STATE;
    const uint32_t G = SOTS_SYNTH_GRAPH;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- the numbers that follow from a mask ----
    CHECK(feedback_gene_count(0) == 0 && feedback_gene_count(0b10) == 1 && feedback_gene_count(0xFF) == 8 && feedback_gene_count(0b10101) == 3);
    CHECK(graph_dims(2, 0) == 4 && graph_dims(2, 0b10) == 5 && graph_dims(2, 0b11) == 6 && graph_dims(5, 0b11111) == 15 && graph_dims(8, 0) == 16);
    CHECK(feedback_gene_column(2, 0b10, 1) == 4 && feedback_gene_column(2, 0b11, 0) == 4 && feedback_gene_column(2, 0b11, 1) == 5);
    CHECK(feedback_gene_column(5, 0b10100, 2) == 10 && feedback_gene_column(5, 0b10100, 4) == 11 && feedback_gene_column(5, 0b11111, 4) == 14);
    // ---- the effective index: NaN, negatives and zeros give +0, values above 2 give 2 ----
    CHECK(same_bits(effective_feedback(0.25f), 0.25f) && same_bits(effective_feedback(2.0f), 2.0f) && same_bits(effective_feedback(1.0f), 1.0f));
    CHECK(same_bits(effective_feedback(3.0f), 2.0f) && same_bits(effective_feedback(inf), 2.0f) && same_bits(effective_feedback(std::nextafterf(2.0f, 3.0f)), 2.0f));
    CHECK(same_bits(effective_feedback(0.0f), 0.0f) && same_bits(effective_feedback(-0.0f), 0.0f) && same_bits(effective_feedback(-1.0f), 0.0f));
    CHECK(same_bits(effective_feedback(-inf), 0.0f) && same_bits(effective_feedback(nan), 0.0f) && same_bits(effective_feedback(-nan), 0.0f));
    CHECK(same_bits(effective_feedback(std::numeric_limits<float>::denorm_min()), std::numeric_limits<float>::denorm_min()));
    // ---- what passes ----
    const sots_voice_graph two = chain(2), five = chain(5), six = chain(6), eight = chain(8);
    sots_config c = config(2, 5);
    CHECK(passes(config_check(c, 1ull << 26, &two, 0b10)));
    c = config(2, 6);
    CHECK(passes(config_check(c, 1ull << 26, &two, 0b11)));
    c = config(5, 15);
    CHECK(passes(config_check(c, kNoPopulationLimit, &five, 0b11111)));
    c = config(6, 16);
    CHECK(passes(config_check(c, kNoPopulationLimit, &six, 0b101011)));
    c = config(5, 11);
    c.param_min[10] = c.param_max[10] = 0.75f; // a range of one value, and the bounds themselves
    CHECK(passes(config_check(c, 1ull << 26, &five, 0b00100)));
    c.param_min[10] = 0.0f, c.param_max[10] = 0.0f;
    CHECK(passes(config_check(c, 1ull << 26, &five, 0b00100)));
    c.param_min[10] = -0.0f, c.param_max[10] = 2.0f;
    CHECK(passes(config_check(c, 1ull << 26, &five, 0b00100)));
    // mask 0: the rules of sots_create_graph, the old text for the old rule
    c = config(2, 4);
    CHECK(passes(config_check(c, 1ull << 26, &two, 0)));
    c = config(2, 5);
    CHECK(refuses(config_check(c, 1ull << 26, &two, 0), inv, "synth_kind 4 needs numDimensions 4, got 5"));
    CHECK(refuses(config_check(c, 1ull << 26, &two), inv, "synth_kind 4 needs numDimensions 4, got 5"));
    // ---- every refusal has its own text ----
    CHECK(refuses(config_check(c, 1ull << 26, &two, 0b100), inv, "voice feedback genes: mask 0x4 has bits beyond operator 1"));
    CHECK(refuses(config_check(c, 1ull << 26, &two, 0x80000001u), inv, "voice feedback genes: mask 0x80000001 has bits beyond operator 1"));
    c = config(8, 16);
    CHECK(refuses(config_check(c, 1ull << 26, &eight, 0x100), inv, "voice feedback genes: mask 0x100 has bits beyond operator 7"));
    CHECK(refuses(config_check(c, 1ull << 26, &eight, 0b1), inv, "voice feedback genes: 8 operators and 1 feedback genes are 17 genes, more than 16"));
    CHECK(refuses(config_check(c, 1ull << 26, &eight, 0xFF), inv, "voice feedback genes: 8 operators and 8 feedback genes are 24 genes, more than 16"));
    c = config(6, 16);
    CHECK(refuses(config_check(c, 1ull << 26, &six, 0b11111), inv, "voice feedback genes: 6 operators and 5 feedback genes are 17 genes, more than 16"));
    c = config(2, 4);
    CHECK(refuses(config_check(c, 1ull << 26, &two, 0b10), inv, "voice feedback genes: 2 operators and 1 feedback genes need numDimensions 5, got 4"));
    c = config(2, 6);
    CHECK(refuses(config_check(c, 1ull << 26, &two, 0b01), inv, "voice feedback genes: 2 operators and 1 feedback genes need numDimensions 5, got 6"));
    c = config(2, 5);
    c.param_max[4] = 2.5f;
    CHECK(refuses(config_check(c, 1ull << 26, &two, 0b10), inv,
                  "voice feedback genes: gene 4 (operator 1's index) has the range 0..2.5, not 0 <= min <= max <= 2"));
    c.param_max[4] = 1.0f, c.param_min[4] = -0.5f;
    CHECK(refuses(config_check(c, 1ull << 26, &two, 0b10), inv,
                  "voice feedback genes: gene 4 (operator 1's index) has the range -0.5..1, not 0 <= min <= max <= 2"));
    c.param_min[4] = 1.5f; // inverted
    CHECK(refuses(config_check(c, 1ull << 26, &two, 0b10), inv,
                  "voice feedback genes: gene 4 (operator 1's index) has the range 1.5..1, not 0 <= min <= max <= 2"));
    c.param_min[4] = 0.0f, c.param_max[4] = inf;
    CHECK(refuses(config_check(c, 1ull << 26, &two, 0b10), inv,
                  "voice feedback genes: gene 4 (operator 1's index) has the range 0..inf, not 0 <= min <= max <= 2"));
    c.param_max[4] = nan;
    CHECK(config_check(c, 1ull << 26, &two, 0b10).code == inv);
    c.param_max[4] = 2.0f, c.param_min[4] = nan;
    CHECK(config_check(c, 1ull << 26, &two, 0b10).code == inv);
    c = config(5, 12);
    c.param_max[11] = 3.0f; // the second gene column is operator 4's
    CHECK(refuses(config_check(c, 1ull << 26, &five, 0b10100), inv,
                  "voice feedback genes: gene 11 (operator 4's index) has the range 0..3, not 0 <= min <= max <= 2"));
    // a graph that is wrong, or no graph voice, is refused with the old texts before the mask is looked at
    c = config(2, 5);
    c.synth_kind = SOTS_SYNTH_2OP;
    CHECK(refuses(config_check(c, 1ull << 26, &two, 0b10), inv, "a voice graph needs synth_kind 4 (SOTS_SYNTH_GRAPH), got 0"));
    c = config(2, 5);
    sots_voice_graph dead = two;
    dead.carriers = 0;
    CHECK(refuses(config_check(c, 1ull << 26, &dead, 0b10), inv, "voice graph: no carrier"));
    // ---- a fixed index on a gene operator ----
    const float three[3] = {0.25f, 0.0f, 2.0f}, zeros[3] = {0.0f, -0.0f, 0.0f};
    float held[8] = {0.5f, 0, 0, 0, 0, 0, 0, 0};
    const float before[8] = {0.5f, 0, 0, 0, 0, 0, 0, 0}, after[8] = {0.25f, 0, 2.0f, 0, 0, 0, 0, 0}, none[8] = {0};
    CHECK(passes(voice_feedback_check(G, 3, three, 3, 0b010)));
    CHECK(passes(voice_feedback_check(G, 3, zeros, 3, 0b111)));
    CHECK(passes(voice_feedback_check(G, 3, nullptr, 0, 0b111)));
    CHECK(refuses(voice_feedback_check(G, 3, three, 3, 0b100), inv,
                  "voice feedback: index 2 for operator 2, whose index is a gene (feedback_genes 0x4): only 0 can be set"));
    CHECK(refuses(voice_feedback_set(G, 3, three, 3, held, 0b001), inv,
                  "voice feedback: index 0.25 for operator 0, whose index is a gene (feedback_genes 0x1): only 0 can be set") &&
          memcmp(held, before, sizeof held) == 0);
    const float out_of_range[3] = {2.5f, 0.0f, 0.0f}; // the older rule speaks first
    CHECK(refuses(voice_feedback_check(G, 3, out_of_range, 3, 0b001), inv, "voice feedback: index 2.5 of operator 0 is outside 0..2"));
    CHECK(passes(voice_feedback_set(G, 3, three, 3, held, 0b010)) && memcmp(held, after, sizeof held) == 0);
    CHECK(passes(voice_feedback_set(G, 3, zeros, 3, held, 0b111)) && memcmp(held, none, sizeof held) == 0);
    // ---- the getter ----
    uint32_t mask = 0;
    CHECK(passes(voice_feedback_genes_get_check(G, &mask)));
    CHECK(refuses(voice_feedback_genes_get_check(SOTS_SYNTH_2OP, &mask), state, "voice feedback genes: the handle runs a fixed voice (synth_kind 0)"));
    CHECK(refuses(voice_feedback_genes_get_check(G, nullptr), inv, "voice feedback genes: null argument"));
    // ---- the two renderers that take beta from the context ----
    sots_render_continuous_args ca{};
    ca.struct_size = sizeof ca;
    ca.hop = 128;
    sots_render_graph_feedback_args fa{};
    fa.struct_size = sizeof fa;
    fa.hop = 128;
    float rows[3 * 5] = {0}, out[512] = {0};
    CHECK(passes(render_graph_continuous_check(G, none, &ca, 256, 5, rows, sizeof rows, 3, out, 512, 0)));
    CHECK(passes(render_graph_feedback_check(G, &fa, 256, 5, rows, sizeof rows, 3, out, 512, 0)));
    CHECK(refuses(render_graph_continuous_check(G, none, &ca, 256, 5, rows, sizeof rows, 3, out, 512, 0b10), state,
                  "sots_render_graph_continuous: the feedback indices of operators 0x2 are genes (sots_create_graph_genes): every row has its "
                  "own; sots_render_overlap_add renders such a voice"));
    CHECK(refuses(render_graph_feedback_check(G, &fa, 256, 5, rows, sizeof rows, 3, out, 512, 0b10), state,
                  "sots_render_graph_feedback: the feedback indices of operators 0x2 are genes (sots_create_graph_genes): every row has its "
                  "own; sots_render_overlap_add renders such a voice"));
    CHECK(refuses(render_graph_feedback_check(SOTS_SYNTH_2OP, &fa, 256, 4, rows, sizeof rows, 3, out, 512, 0b10), state,
                  "sots_render_graph_feedback: the handle runs a fixed voice (synth_kind 0; sots_render_continuous renders it)"));

    printf("graph feedback genes: %d checks, %d failures\n", checks, bad);
    return bad != 0;
}
