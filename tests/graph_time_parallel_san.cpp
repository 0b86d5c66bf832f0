// graph_time_parallel_san.cpp -- the plan of the graph voice's time-parallel synthesis form (csrc/sots_rules.h:
// graph_tp_plan, graph_synth_form_for) over the thirteen graphs of the tests and over every legal graph of 2, 3 and 4
// operators: the schedule keeps its own constraints, buffer regions never overlap and stay inside the 31 KiB, and a replay
// of the schedule, tick by tick, finds in every ring slot and phase buffer the block its reader expects, with no slot read
// and written in one tick.  Built and run by tests/test_graph_time_parallel_cpu.py under ASan + UBSan; host code only, no
// HIP header.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
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

static sots_voice_graph graph(uint32_t ops, uint32_t carriers, const uint32_t *mods)
{
    sots_voice_graph g;
    memset(&g, 0, sizeof g);
    g.struct_size = sizeof g;
    g.num_operators = ops;
    g.carriers = carriers;
    for (uint32_t j = 0; j < ops && j < 8; ++j) g.modulators[j] = mods[j];
    return g;
}

// everything that must hold for the plan of a checked graph
static void check_plan(const sots_voice_graph &g)
{
    const GraphTpPlan p = graph_tp_plan(g);
    const GraphLevels lv = graph_levels(g);
    const uint32_t ops = g.num_operators;
    CHECK(p.ops == ops && p.levels == lv.count);
    CHECK(p.evaluators >= 1 && ops * (1 + p.evaluators) <= 16); // at most 1024 threads
    CHECK((g.carriers >> p.mixer & 1u) && p.depth[p.mixer] == 0 && p.lag == p.tick_of[p.mixer] + 1);
    uint32_t carriers = 0, rows = 2 * ops;
    for (uint32_t j = 0; j < ops; ++j) {
        carriers += g.carriers >> j & 1u;
        rows += p.depth[j];
        CHECK(p.tick_of[j] >= 2 * lv.level_of[j]);
        for (uint32_t i = 0; i < j; ++i)
            if (g.modulators[j] >> i & 1u) CHECK(p.tick_of[j] >= p.tick_of[i] + 2);
        if ((g.carriers >> j & 1u) && j != p.mixer) CHECK(p.tick_of[p.mixer] > p.tick_of[j]);
    }
    CHECK(carriers == p.num_carriers && rows == p.rows);
    // the bytes: whole rows of every individual, within the 31 KiB, and one more individual would not fit
    const uint32_t per_individual = p.rows * kGraphTpRow * 4;
    CHECK(graph_tp_bytes(p) == per_individual * p.capacity && graph_tp_bytes(p) <= 31u * 1024u);
    CHECK(p.capacity == 64 || per_individual * (p.capacity + 1) > 31u * 1024u);
    if (p.capacity == 0) return;
    // the regions: [first, end) in floats, pairwise disjoint, inside the buffer, 16-byte aligned
    std::vector<std::pair<uint32_t, uint32_t>> regions;
    for (uint32_t j = 0; j < ops; ++j) {
        regions.push_back({p.phase_off[j], p.phase_off[j] + 2 * p.capacity * kGraphTpRow});
        if (p.depth[j]) regions.push_back({p.ring_off[j], p.ring_off[j] + p.depth[j] * p.capacity * kGraphTpRow});
    }
    bool disjoint = true, inside = true;
    for (size_t a = 0; a < regions.size(); ++a) {
        inside = inside && regions[a].second <= kGraphTpLdsBytes / 4 && regions[a].first % 4 == 0;
        for (size_t b = a + 1; b < regions.size(); ++b)
            disjoint = disjoint && (regions[a].second <= regions[b].first || regions[b].second <= regions[a].first);
    }
    CHECK(disjoint);
    CHECK(inside);
    // the replay: 4 blocks (fewer than a deep pipeline holds) and 40; slot contents are block numbers
    for (uint32_t blocks : {4u, 40u}) {
        std::vector<std::vector<int64_t>> ring(ops), phase(ops, std::vector<int64_t>(2, -1));
        for (uint32_t j = 0; j < ops; ++j) ring[j].assign(p.depth[j] ? p.depth[j] : 1, -1);
        bool found = true, clash = false;
        uint64_t audio_blocks = 0;
        for (uint32_t tick = 0; tick < blocks + p.lag; ++tick) {
            std::vector<std::vector<char>> ring_read(ops), phase_read(ops, std::vector<char>(2, 0));
            for (uint32_t j = 0; j < ops; ++j) ring_read[j].assign(ring[j].size(), 0);
            // reads of this tick (a scan's own in-place phase block is written before it is read, by one wavefront)
            for (uint32_t j = 0; j < ops; ++j) {
                const uint32_t ks = tick - p.tick_of[j], ke = tick - p.tick_of[j] - 1;
                if (ks < blocks)
                    for (uint32_t i = 0; i < j; ++i)
                        if (g.modulators[j] >> i & 1u) {
                            found = found && p.depth[i] && ring[i][ks % p.depth[i]] == (int64_t)ks;
                            if (p.depth[i]) ring_read[i][ks % p.depth[i]] = 1;
                        }
                if (ke < blocks) {
                    found = found && phase[j][ke & 1] == (int64_t)ke;
                    phase_read[j][ke & 1] = 1;
                    if (j == p.mixer) {
                        ++audio_blocks;
                        for (uint32_t i = 0; i < ops; ++i)
                            if ((g.carriers >> i & 1u) && i != j) {
                                found = found && p.depth[i] && ring[i][ke % p.depth[i]] == (int64_t)ke;
                                if (p.depth[i]) ring_read[i][ke % p.depth[i]] = 1;
                            }
                    }
                }
            }
            // writes of this tick
            for (uint32_t j = 0; j < ops; ++j) {
                const uint32_t ks = tick - p.tick_of[j], ke = tick - p.tick_of[j] - 1;
                if (ks < blocks) {
                    clash = clash || phase_read[j][ks & 1];
                    phase[j][ks & 1] = ks;
                }
                if (ke < blocks && j != p.mixer) {
                    clash = clash || p.depth[j] == 0 || ring_read[j][ke % ring[j].size()];
                    ring[j][ke % ring[j].size()] = ke;
                }
            }
        }
        CHECK(found);
        CHECK(!clash);
        CHECK(audio_blocks == blocks);
    }
}

int main()
{
    // ---- the thirteen graphs of tests/_graph_voice_model.py: capacity, levels, ticks ----
    struct Named {
        const char *name;
        uint32_t ops, carriers, mods[8], capacity, levels;
    };
    const Named named[] = {
        {"2op", 2, 0b10, {0, 1}, 19, 2},
        {"triple", 6, 0b101010, {0, 1, 0, 4, 0, 16}, 5, 2},
        {"chain3", 3, 0b100, {0, 1, 2}, 11, 3},
        {"two_mods", 3, 0b100, {0, 0, 3}, 11, 2},
        {"one_mod_two_carriers", 3, 0b110, {0, 1, 1}, 10, 2},
        {"additive", 2, 0b11, {0, 0}, 19, 1},
        {"chain8", 8, 0x80, {0, 1, 2, 4, 8, 16, 32, 64}, 3, 8},
        {"fan3", 4, 0b1000, {0, 0, 0, 7}, 8, 2},
        {"stacks5", 5, 0b10100, {0, 1, 2, 0, 8}, 6, 3},
        {"seven", 7, 0b1000100, {0, 1, 2, 0, 0, 0, 0b0111000}, 4, 3},
        {"dense8", 8, 0xC0, {0, 1, 3, 7, 15, 31, 63, 63}, 1, 7},
        {"additive8", 8, 0xFF, {0, 0, 0, 0, 0, 0, 0, 0}, 3, 1},
        {"one_to_seven", 8, 0xFE, {0, 1, 1, 1, 1, 1, 1, 1}, 3, 2},
    };
    for (const Named &n : named) {
        const sots_voice_graph g = graph(n.ops, n.carriers, n.mods);
        CHECK(!voice_graph_check(&g));
        const GraphTpPlan p = graph_tp_plan(g);
        if (p.capacity != n.capacity || p.levels != n.levels) printf("  %s: capacity %u levels %u rows %u\n", n.name, p.capacity, p.levels, p.rows);
        CHECK(p.capacity == n.capacity && p.levels == n.levels);
        if (n.ops <= 4) CHECK(p.capacity >= 8); // the shipped workload's share of a CU
        check_plan(g);
    }
    // ---- every legal graph of 2, 3 and 4 operators ----
    uint32_t legal = 0;
    for (uint32_t ops = 2; ops <= 4; ++ops) {
        uint32_t combos = 1;
        for (uint32_t j = 0; j < ops; ++j) combos <<= j; // modulators[j]: any mask of the operators below j
        for (uint32_t code = 0; code < combos; ++code)
            for (uint32_t carriers = 1; carriers < (1u << ops); ++carriers) {
                uint32_t mods[8] = {0}, rest = code;
                for (uint32_t j = 0; j < ops; ++j) mods[j] = rest & ((1u << j) - 1u), rest >>= j;
                const sots_voice_graph g = graph(ops, carriers, mods);
                if (voice_graph_check(&g)) continue;
                ++legal;
                check_plan(g);
                CHECK(graph_tp_plan(g).capacity >= 1);
            }
    }
    CHECK(legal > 20);
    // ---- the choice rule: what keeps the lane form whatever is asked for ----
    {
        const sots_voice_graph g = graph(2, 0b10, named[0].mods);
        const float none[8] = {0}, some[8] = {0, 0.5f};
        const uint32_t lanes = SOTS_GRAPH_FORM_LANES, tp = SOTS_GRAPH_FORM_TIME_PARALLEL;
        CHECK(graph_synth_form_for(tp, g, none, 0, 1024, 256) == tp);
        CHECK(graph_synth_form_for(tp, g, nullptr, 0, 1u << 20, 256) == tp); // any population when forced
        CHECK(graph_synth_form_for(tp, g, some, 0, 1024, 256) == lanes);
        CHECK(graph_synth_form_for(tp, g, none, 0b10, 1024, 256) == lanes);
        CHECK(graph_synth_form_for(lanes, g, none, 0, 32, 256) == lanes);
        CHECK(graph_synth_form_for(SOTS_GRAPH_FORM_AUTO, g, none, 0, 65536, 256) == lanes); // 256 per CU: beyond any capacity
        CHECK(graph_synth_form_for(SOTS_GRAPH_FORM_AUTO, g, none, 0, 1024, 256) == tp);      // 4 per CU
        CHECK(graph_synth_form_for(SOTS_GRAPH_FORM_AUTO, g, none, 0, 19 * 256, 256) == tp && graph_synth_form_for(SOTS_GRAPH_FORM_AUTO, g, none, 0, 19 * 256 + 1, 256) == lanes);
        CHECK(graph_synth_form_for(SOTS_GRAPH_FORM_AUTO, g, some, 0, 32, 256) == lanes);
        CHECK(graph_synth_form_check(SOTS_SYNTH_2OP, 0).code == SOTS_ERR_STATE);
        CHECK(graph_synth_form_check(SOTS_SYNTH_GRAPH, 3).code == SOTS_ERR_INVALID);
        CHECK(!graph_synth_form_check(SOTS_SYNTH_GRAPH, 2));
    }
    printf("graph time parallel: %u legal graphs, %d checks, %d failures\n", legal, checks, bad);
    return bad ? 1 : 0;
}
