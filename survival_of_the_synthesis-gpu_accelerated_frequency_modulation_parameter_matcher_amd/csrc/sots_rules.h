// sots_rules.h -- what a context (sots_ctx), a batch (sots_batch) and a group accept, and the numbers that follow from a
// configuration, stated ONCE: the handles call these and add their own limits.  A refusal is a Fault: the code the entry
// point returns and the text its last_error gives.  No HIP header: plain C++ compilers build it too (the sanitizer
// builds of tests/).  Internal to libsots_hip.so.
#pragma once

#include <stdint.h>

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <vector>

#include "../../include/sots_hip.h"

namespace sots {

struct Fault {
    int code = SOTS_OK;
    char text[512] = {0};
    explicit operator bool() const { return code != SOTS_OK; }
};
__attribute__((format(printf, 2, 3))) inline Fault fault(int code, const char *fmt, ...)
{
    Fault f;
    f.code = code;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(f.text, sizeof f.text, fmt, ap);
    va_end(ap);
    return f;
}

// ---- configuration ----
// genes of a voice; 0: no such voice
inline uint32_t dims_of(uint32_t kind)
{
    switch (kind) {
    case SOTS_SYNTH_2OP: return 4;
    case SOTS_SYNTH_3OP_SERIES: return 6;
    case SOTS_SYNTH_TRIPLE_PAR: return 12;
    case SOTS_SYNTH_4OP_SERIES: return 8;
    default: return 0;
    }
}

// ---- operator-graph voice (SOTS_SYNTH_GRAPH; the definition: include/sots_hip.h) ----
constexpr uint32_t kGraphMinOps = 2, kGraphMaxOps = 8;
// operators that operator j's output modulates, as a bit mask (bits above j)
inline uint32_t graph_targets_of(const sots_voice_graph &g, uint32_t j)
{
    uint32_t t = 0;
    for (uint32_t k = j + 1; k < g.num_operators && k < kGraphMaxOps; ++k)
        if (g.modulators[k] >> j & 1u) t |= 1u << k;
    return t;
}
// A feed-forward graph in which every operator is heard or modulates, never both and never neither
inline Fault voice_graph_check(const sots_voice_graph *g)
{
    if (!g) return fault(SOTS_ERR_INVALID, "voice graph: null pointer");
    if (g->struct_size != sizeof(sots_voice_graph))
        return fault(SOTS_ERR_INVALID, "sots_voice_graph.struct_size %u != %zu", g->struct_size, sizeof(sots_voice_graph));
    const uint32_t ops = g->num_operators;
    if (ops < kGraphMinOps || ops > kGraphMaxOps)
        return fault(SOTS_ERR_INVALID, "voice graph: %u operators outside %u..%u", ops, kGraphMinOps, kGraphMaxOps);
    const uint32_t all = (1u << ops) - 1u;
    if (g->carriers & ~all) return fault(SOTS_ERR_INVALID, "voice graph: carriers 0x%x has bits beyond operator %u", g->carriers, ops - 1u);
    for (uint32_t j = ops; j < kGraphMaxOps; ++j)
        if (g->modulators[j]) return fault(SOTS_ERR_INVALID, "voice graph: modulators[%u] = 0x%x beyond operator %u", j, g->modulators[j], ops - 1u);
    for (uint32_t j = 0; j < ops; ++j)
        if (g->modulators[j] >> j)
            return fault(SOTS_ERR_INVALID, "voice graph: modulators[%u] = 0x%x has a bit at or above %u (feed-forward only: operator i < j modulates j)",
                         j, g->modulators[j], j);
    if (g->carriers == 0) return fault(SOTS_ERR_INVALID, "voice graph: no carrier");
    for (uint32_t j = 0; j < ops; ++j) {
        const bool carrier = g->carriers >> j & 1u, modulates = graph_targets_of(*g, j) != 0;
        if (carrier && modulates) return fault(SOTS_ERR_INVALID, "voice graph: operator %u is a carrier and modulates (one or the other)", j);
        if (!carrier && !modulates) return fault(SOTS_ERR_INVALID, "voice graph: operator %u is dead: neither a carrier nor a modulator", j);
    }
    return Fault{};
}

// ---- operator waveforms of the graph voice (sots_set_voice_waveforms; the definition: include/sots_hip.h) ----
constexpr uint32_t kWaveformCount = 8;
// codes[count] for a handle of synthesis kind `kind` whose graph has `ops` operators; (null, 0): all sine
inline Fault voice_waveforms_check(uint32_t kind, uint32_t ops, const uint32_t *codes, uint32_t count)
{
    if (kind != SOTS_SYNTH_GRAPH)
        return fault(SOTS_ERR_STATE, "voice waveforms: the handle runs a fixed voice (synth_kind %u)", kind);
    if (!codes && count == 0) return Fault{};
    if (!codes) return fault(SOTS_ERR_INVALID, "voice waveforms: null codes with a count of %u", count);
    if (count != ops) return fault(SOTS_ERR_INVALID, "voice waveforms: %u codes for a graph of %u operators", count, ops);
    for (uint32_t j = 0; j < count; ++j)
        if (codes[j] >= kWaveformCount)
            return fault(SOTS_ERR_INVALID, "voice waveforms: code %u of operator %u is not a waveform (0..%u)", codes[j], j, kWaveformCount - 1u);
    return Fault{};
}
// What the shaped kernel takes: 3 bits per operator, operator j in bits 3j..3j+2.  0: all sine.
inline uint32_t pack_waveforms(const uint32_t codes[8])
{
    uint32_t packed = 0;
    for (uint32_t j = 0; j < kGraphMaxOps; ++j) packed |= (codes[j] & 7u) << (3u * j);
    return packed;
}
inline void unpack_waveforms(uint32_t packed, uint32_t codes[8])
{
    for (uint32_t j = 0; j < kGraphMaxOps; ++j) codes[j] = packed >> (3u * j) & 7u;
}
// Checks, then writes all eight codes of `held` (0 beyond the operators); a refusal leaves `held` as it was
inline Fault voice_waveforms_set(uint32_t kind, uint32_t ops, const uint32_t *codes, uint32_t count, uint32_t held[8])
{
    if (const Fault f = voice_waveforms_check(kind, ops, codes, count)) return f;
    for (uint32_t j = 0; j < kGraphMaxOps; ++j) held[j] = codes && j < count ? codes[j] : 0u;
    return Fault{};
}

// ---- per-operator feedback of the graph voice (sots_set_voice_feedback; the definition: include/sots_hip.h) ----
constexpr float kFeedbackMax = 2.0f;
// K of the definition: the fp32 nearest W / 2 pi, table entries per unit of h at an index of 1
constexpr float kFeedbackScale = 0x1.45f306p+12f;
// index[count] for a handle of synthesis kind `kind` whose graph has `ops` operators; (null, 0): no feedback.
// feedback_genes: the operators whose index is a gene of the individual (sots_create_graph_genes): theirs stays 0 here
inline Fault voice_feedback_check(uint32_t kind, uint32_t ops, const float *index, uint32_t count, uint32_t feedback_genes = 0)
{
    if (kind != SOTS_SYNTH_GRAPH)
        return fault(SOTS_ERR_STATE, "voice feedback: the handle runs a fixed voice (synth_kind %u)", kind);
    if (!index && count == 0) return Fault{};
    if (!index) return fault(SOTS_ERR_INVALID, "voice feedback: null indices with a count of %u", count);
    if (count != ops) return fault(SOTS_ERR_INVALID, "voice feedback: %u indices for a graph of %u operators", count, ops);
    for (uint32_t j = 0; j < count; ++j)
        if (!(index[j] >= 0.0f && index[j] <= kFeedbackMax)) // (NaN fails both; -0 >= 0 holds)
            return fault(SOTS_ERR_INVALID, "voice feedback: index %g of operator %u is outside 0..%g", (double)index[j], j, (double)kFeedbackMax);
    for (uint32_t j = 0; j < count; ++j)
        if ((feedback_genes >> j & 1u) && index[j] != 0.0f)
            return fault(SOTS_ERR_INVALID, "voice feedback: index %g for operator %u, whose index is a gene (feedback_genes 0x%x): only 0 can be set",
                         (double)index[j], j, feedback_genes);
    return Fault{};
}
// Checks, then writes all eight indices of `held` (+0 beyond the operators and for -0); a refusal leaves `held` as it was
inline Fault voice_feedback_set(uint32_t kind, uint32_t ops, const float *index, uint32_t count, float held[8], uint32_t feedback_genes = 0)
{
    if (const Fault f = voice_feedback_check(kind, ops, index, count, feedback_genes)) return f;
    for (uint32_t j = 0; j < kGraphMaxOps; ++j) held[j] = index && j < count && index[j] != 0.0f ? index[j] : 0.0f;
    return Fault{};
}
// What the feedback kernel takes: B_j = beta_j K, one fp32 product each (this header is built uncontracted wherever it is
// used, and a lone product has nothing to contract with); returns whether any operator feeds back
inline bool scale_feedback(const float index[8], uint32_t ops, float scaled[8])
{
    bool any = false;
    for (uint32_t j = 0; j < kGraphMaxOps; ++j) {
        const float b = j < ops ? index[j] : 0.0f;
        scaled[j] = b * kFeedbackScale;
        any = any || b != 0.0f;
    }
    return any;
}

// ---- feedback indices as genes (sots_create_graph_genes; the definition: include/sots_hip.h) ----
inline uint32_t feedback_gene_count(uint32_t feedback_genes)
{
    uint32_t e = 0;
    for (uint32_t j = 0; j < kGraphMaxOps; ++j) e += feedback_genes >> j & 1u;
    return e;
}
// genes of a graph voice of `ops` operators whose mask is feedback_genes (a checked mask: nothing beyond the operators)
inline uint32_t graph_dims(uint32_t ops, uint32_t feedback_genes) { return 2u * ops + feedback_gene_count(feedback_genes); }
// the column of operator j's index (bit j of a checked mask is set): 2 OPS + the number of set bits below j
inline uint32_t feedback_gene_column(uint32_t ops, uint32_t feedback_genes, uint32_t j)
{
    return 2u * ops + feedback_gene_count(feedback_genes & ((1u << j) - 1u));
}
// The effective index of a scaled gene p: NaN and everything not above 0 give +0, everything above 2 gives 2
// (constexpr: the renderer's chain kernels make it per sample, sots_render_graph.hip)
constexpr float effective_feedback(float p) { return p > 0.0f ? (p < kFeedbackMax ? p : kFeedbackMax) : 0.0f; }
// What a mask other than 0 adds to config_check, for a checked graph: the mask lies within the operators, the genes fit a
// row, the configuration counts them, and each gene column's range lies in [0, 2] in ascending order
inline Fault voice_feedback_genes_check(const sots_config &cfg, const sots_voice_graph &graph, uint32_t feedback_genes)
{
    const uint32_t ops = graph.num_operators;
    if (feedback_genes >> ops)
        return fault(SOTS_ERR_INVALID, "voice feedback genes: mask 0x%x has bits beyond operator %u", feedback_genes, ops - 1u);
    const uint32_t e = feedback_gene_count(feedback_genes), d = 2u * ops + e;
    if (d > SOTS_MAX_DIMS)
        return fault(SOTS_ERR_INVALID, "voice feedback genes: %u operators and %u feedback genes are %u genes, more than %u", ops, e, d,
                     (uint32_t)SOTS_MAX_DIMS);
    if (cfg.num_dimensions != d)
        return fault(SOTS_ERR_INVALID, "voice feedback genes: %u operators and %u feedback genes need numDimensions %u, got %u", ops, e, d,
                     cfg.num_dimensions);
    for (uint32_t j = 0; j < ops; ++j) {
        if (!(feedback_genes >> j & 1u)) continue;
        const uint32_t g = feedback_gene_column(ops, feedback_genes, j);
        const float lo = cfg.param_min[g], hi = cfg.param_max[g];
        if (!(lo >= 0.0f && lo <= hi && hi <= kFeedbackMax)) // (false for NaN)
            return fault(SOTS_ERR_INVALID, "voice feedback genes: gene %u (operator %u's index) has the range %g..%g, not 0 <= min <= max <= %g", g, j,
                         (double)lo, (double)hi, (double)kFeedbackMax);
    }
    return Fault{};
}
// the getter's rule
inline Fault voice_feedback_genes_get_check(uint32_t kind, const void *out)
{
    if (kind != SOTS_SYNTH_GRAPH)
        return fault(SOTS_ERR_STATE, "voice feedback genes: the handle runs a fixed voice (synth_kind %u)", kind);
    if (!out) return fault(SOTS_ERR_INVALID, "voice feedback genes: null argument");
    return Fault{};
}

// Everything a configuration must satisfy whoever takes it; max_population is the caller's own limit on numParents +
// numOffspring.  Needs no device: a machine without a GPU still tells a bad configuration from a good one.  graph: the
// topology that came with the configuration (sots_create_graph, sots_batch_create_graph), null from every other entry point.
// feedback_genes: the mask of sots_create_graph_genes / sots_batch_create_graph_genes, 0 from every other entry point.
constexpr uint64_t kNoPopulationLimit = ~0ull; // (a caller that words its limit itself)
inline Fault config_check(const sots_config &cfg, uint64_t max_population, const sots_voice_graph *graph = nullptr, uint32_t feedback_genes = 0)
{
    if (cfg.struct_size != sizeof(sots_config))
        return fault(SOTS_ERR_INVALID, "sots_config.struct_size %u != %zu", cfg.struct_size, sizeof(sots_config));
    if (graph && cfg.synth_kind != SOTS_SYNTH_GRAPH)
        return fault(SOTS_ERR_INVALID, "a voice graph needs synth_kind %u (SOTS_SYNTH_GRAPH), got %u", (uint32_t)SOTS_SYNTH_GRAPH, cfg.synth_kind);
    if (!graph && cfg.synth_kind == SOTS_SYNTH_GRAPH)
        return fault(SOTS_ERR_INVALID, "synth_kind %u (SOTS_SYNTH_GRAPH) needs its topology: sots_create_graph / sots_batch_create_graph",
                     cfg.synth_kind);
    if (graph)
        if (const Fault f = voice_graph_check(graph)) return f;
    if (graph && feedback_genes)
        if (const Fault f = voice_feedback_genes_check(cfg, *graph, feedback_genes)) return f;
    const uint32_t d = graph ? graph_dims(graph->num_operators, feedback_genes) : dims_of(cfg.synth_kind);
    if (d == 0) return fault(SOTS_ERR_INVALID, "unknown synth_kind %u", cfg.synth_kind);
    if (cfg.num_dimensions != d)
        return fault(SOTS_ERR_INVALID, "synth_kind %u needs numDimensions %u, got %u", cfg.synth_kind, d, cfg.num_dimensions);
    if (cfg.audio_length_log2 < 8 || cfg.audio_length_log2 > 15)
        return fault(SOTS_ERR_INVALID, "audioLengthLog2 %u outside 8..15", cfg.audio_length_log2);
    const uint64_t p64 = (uint64_t)cfg.num_parents + cfg.num_offspring;
    if (cfg.num_parents == 0 || p64 < 2 || p64 > max_population)
        return fault(SOTS_ERR_INVALID, "population %llu (parents %u) not supported", (unsigned long long)p64, cfg.num_parents);
    if (cfg.workgroup_size == 0 || p64 % cfg.workgroup_size != 0)
        return fault(SOTS_ERR_INVALID, "populationLength %llu must be a multiple of workgroupSize %u (the recombination block)",
                     (unsigned long long)p64, cfg.workgroup_size);
    return Fault{};
}

// sots_set_synth_arithmetic: the reference's device kernels exist for its own three voices only
inline Fault synth_arithmetic_check(uint32_t arith, uint32_t kind)
{
    if (arith > SOTS_ARITH_DEVICE_KERNELS) return fault(SOTS_ERR_INVALID, "unknown synthesis arithmetic %u", arith);
    if (arith == SOTS_ARITH_DEVICE_KERNELS && kind == SOTS_SYNTH_4OP_SERIES)
        return fault(SOTS_ERR_INVALID, "the reference has no device kernel for the build-defined 4-op voice");
    if (arith == SOTS_ARITH_DEVICE_KERNELS && kind == SOTS_SYNTH_GRAPH)
        return fault(SOTS_ERR_INVALID, "the reference has no device kernel for the operator-graph voice");
    return Fault{};
}

// ES constants, Evolutionary_Strategy.hpp:611-627; the two pow(Ek, beta) values are
// evaluated once on the host (Ek only ever takes two values, ocl_program.cl:168,185).
struct MutateConsts {
    float alpha, one_over_alpha, root_two_over_pi, beta_scale;
    float pow_alpha_beta, pow_inv_alpha_beta;
};
inline MutateConsts mutate_consts(uint32_t num_dimensions)
{
    const float mpi = (float)3.14159265358979323846;
    MutateConsts mc;
    mc.alpha = 1.4f;
    mc.one_over_alpha = 1.f / mc.alpha;
    mc.root_two_over_pi = sqrtf(2.f / (float)mpi);
    mc.beta_scale = 1.f / (float)num_dimensions;
    const float beta = sqrtf(mc.beta_scale);
    mc.pow_alpha_beta = powf(mc.alpha, beta);
    mc.pow_inv_alpha_beta = powf(mc.one_over_alpha, beta);
    return mc;
}

// ---- the rows of a sorted half ----
// Rows that the next recombination reads (recombine_source, kernels/variation.h):
// whole blocks of parents, floor(numParents / block) of them, at least one.  Immigrants go to the
// tail of THESE rows: with numParents not a multiple of the block, rows between the last whole
// block and numParents are never read and immigrants written there would be dead.
inline uint32_t breeding_rows(uint32_t num_parents, uint32_t block)
{
    if (block == 0) block = 1;
    uint32_t npb = num_parents / block;
    if (npb == 0) npb = 1;
    return npb * block;
}

// rows the selection must deliver in order: what recombination reads, and never fewer than the parents
inline uint32_t selected_rows(uint32_t num_parents, uint32_t block)
{
    const uint32_t b = breeding_rows(num_parents, block);
    return b > num_parents ? b : num_parents;
}

// one population through the C-ABI: P x D floats of values and of steps, P of fitness; an array that is not passed is not counted
inline Fault population_bytes_check(uint32_t p, uint32_t d, const void *values, size_t values_bytes, const void *steps, size_t steps_bytes,
                                    const void *fitness, size_t fitness_bytes)
{
    const size_t pd_bytes = (size_t)p * d * sizeof(float), f_bytes = (size_t)p * sizeof(float);
    if ((values && values_bytes != pd_bytes) || (steps && steps_bytes != pd_bytes) || (fitness && fitness_bytes != f_bytes))
        return fault(SOTS_ERR_SIZE, "population byte counts must be %zu (values, steps) and %zu (fitness)", pd_bytes, f_bytes);
    return Fault{};
}

// ---- objective ----
// 1e-30 <= floor <= 1: m + floor is then a normal fp32 number for every magnitude m >= 0
inline bool objective_floor_ok(float floor) { return floor >= 1e-30f && floor <= 1.0f; } // (false for NaN)
inline Fault objective_check(uint32_t objective, float floor)
{
    if (objective != SOTS_OBJECTIVE_MAGNITUDE && objective != SOTS_OBJECTIVE_LOG_MAGNITUDE)
        return fault(SOTS_ERR_INVALID, "unknown objective %u (0 = magnitude, 1 = log magnitude)", objective);
    if (objective == SOTS_OBJECTIVE_LOG_MAGNITUDE && !objective_floor_ok(floor))
        return fault(SOTS_ERR_INVALID, "log-magnitude floor %g outside 1e-30 .. 1", (double)floor);
    return Fault{};
}

// w[n] as sots_set_objective_weights takes it: n == bins, every entry finite and >= 0, one at least > 0.  0: fine, and
// u[k] = sqrtf(w[k]) (correctly rounded); 1: wrong length; 2: entry *bad is negative or not finite; 3: all zero
inline int objective_weights_check(const float *w, uint32_t n, uint32_t bins, std::vector<float> &u, uint32_t *bad)
{
    if (n != bins) return 1;
    bool any = false;
    for (uint32_t k = 0; k < n; ++k) {
        if (!(w[k] >= 0.0f) || !std::isfinite(w[k])) return *bad = k, 2;
        any = any || w[k] > 0.0f;
    }
    if (!any) return 3;
    u.resize(n);
    for (uint32_t k = 0; k < n; ++k) u[k] = std::sqrt(w[k]);
    return 0;
}
// ... as a refusal: a table and its length (u as above), or NULL and 0 (no weights, u untouched)
inline Fault objective_weights_fault(const float *weights, uint32_t num_bins, uint32_t bins, std::vector<float> &u)
{
    if ((weights == nullptr) != (num_bins == 0)) return fault(SOTS_ERR_INVALID, "objective weights: a table and its length, or NULL and 0");
    if (!weights) return Fault{};
    uint32_t bad = 0;
    switch (objective_weights_check(weights, num_bins, bins, u, &bad)) {
    case 1: return fault(SOTS_ERR_INVALID, "objective weights need %u bins, got %u", bins, num_bins);
    case 2: return fault(SOTS_ERR_INVALID, "objective weight %u is %g: every weight must be finite and >= 0", bad, (double)weights[bad]);
    case 3: return fault(SOTS_ERR_INVALID, "objective weights are all zero");
    default: return Fault{};
    }
}

// ---- analysis on the device (sots_batch_set_analysis, sots_batch_analyse_audio_hop) ----
inline Fault analysis_mode_check(uint32_t mode)
{
    if (mode != SOTS_ANALYSIS_HOST && mode != SOTS_ANALYSIS_DEVICE)
        return fault(SOTS_ERR_INVALID, "unknown analysis mode %u (0 = host, 1 = device)", mode);
    return Fault{};
}
constexpr uint64_t kAnalysisMaxSamples = 1ull << 28;     // one upload
constexpr uint64_t kAnalysisMaxSpectrumBytes = 1ull << 30; // frames x N/2 magnitudes: the bound of the queue's stored targets
// samples that `frames` (>= 1) frames of n at a hop cover; 64-bit throughout: frames up to 2^32 - 1, hop up to 2^15
inline uint64_t analysis_samples(uint32_t frames, uint32_t hop, uint32_t n) { return (uint64_t)(frames - 1u) * hop + n; }
// What the device analysis refuses before anything touches the device: frames of n samples at a hop out of num_samples
// of audio, one result per frame (or frames x n/2, the caller's own check) into out.  who: the entry point, for the text.
inline Fault analysis_frames_check(const char *who, const void *audio, uint64_t num_samples, uint32_t hop, uint32_t frames, const void *out, uint32_t n)
{
    if (!audio || !out) return fault(SOTS_ERR_INVALID, "%s: null pointer", who);
    if (hop == 0 || hop > n) return fault(SOTS_ERR_INVALID, "%s: hop %u outside 1..%u", who, hop, n);
    if (frames == 0) return fault(SOTS_ERR_INVALID, "%s: the frame count must be at least 1", who);
    const uint64_t need = analysis_samples(frames, hop, n), bytes = (uint64_t)frames * (n / 2u) * sizeof(float);
    if (need > kAnalysisMaxSamples)
        return fault(SOTS_ERR_INVALID, "%s: %u frames at hop %u cover %llu samples, more than %llu", who, frames, hop, (unsigned long long)need,
                     (unsigned long long)kAnalysisMaxSamples);
    if (bytes > kAnalysisMaxSpectrumBytes)
        return fault(SOTS_ERR_INVALID, "%s: %u frames of %u bins exceed %llu bytes of spectra", who, frames, n / 2u,
                     (unsigned long long)kAnalysisMaxSpectrumBytes);
    if (num_samples < need)
        return fault(SOTS_ERR_SIZE, "%s: %u frames at hop %u need %llu samples, got %llu", who, frames, hop, (unsigned long long)need,
                     (unsigned long long)num_samples);
    return Fault{};
}

// ---- phase-continuous rendering ----
// its scans are written per fixed voice: the operator-graph voice has sots_render_graph_continuous (below)
inline Fault render_continuous_voice_check(uint32_t kind)
{
    if (kind == SOTS_SYNTH_GRAPH)
        return fault(SOTS_ERR_INVALID, "sots_render_continuous: not for the operator-graph voice (sots_render_overlap_add renders it)");
    return Fault{};
}
// What the three phase-continuous entry points refuse alike, in two pieces, since an entry point may have refusals of its own
// between them.  who, args_type: the entry point's name and its args struct's, for the text; n, d: the context's audio length
// and genes per row.  The first piece: the args struct, the hop, the flags.
template <class ARGS> inline Fault render_cont_args_check(const char *who, const char *args_type, const ARGS *args, uint32_t n)
{
    if (!args || args->struct_size != sizeof(ARGS)) return fault(SOTS_ERR_INVALID, "%s: null args or %s.struct_size != %zu", who, args_type, sizeof(ARGS));
    if (args->hop < 1u || args->hop > n) return fault(SOTS_ERR_INVALID, "%s: hop %u outside 1..%u", who, args->hop, n);
    if (args->flags & ~(uint32_t)SOTS_RENDER_GLIDE) return fault(SOTS_ERR_INVALID, "%s: unknown flags 0x%x", who, args->flags);
    return Fault{};
}
// The second piece: the rows, the samples they cover, the values and the output.
inline Fault render_cont_track_check(const char *who, uint32_t hop, uint32_t n, uint32_t d, const void *values, size_t values_bytes, uint32_t num_rows,
                                     const void *out, uint64_t out_samples)
{
    if (num_rows == 0) return fault(SOTS_ERR_INVALID, "%s: num_rows must be at least 1", who);
    const uint64_t covered = (uint64_t)(num_rows - 1u) * hop + n;
    if (covered >= (1ull << 31))
        return fault(SOTS_ERR_INVALID, "%s: %u rows at hop %u are %llu samples, 2^31 or more", who, num_rows, hop, (unsigned long long)covered);
    if (!values || values_bytes != (size_t)num_rows * d * sizeof(float))
        return fault(SOTS_ERR_SIZE, "%s: %u rows need %zu bytes of values, got %zu", who, num_rows, (size_t)num_rows * d * sizeof(float), values_bytes);
    if (!out && out_samples) return fault(SOTS_ERR_INVALID, "%s: null output", who);
    return Fault{};
}
// The graph voice's two entry points refuse a fixed voice and a voice whose feedback indices are genes before they look at args.
inline Fault render_graph_voice_check(const char *who, uint32_t kind, uint32_t feedback_genes)
{
    if (kind != SOTS_SYNTH_GRAPH)
        return fault(SOTS_ERR_STATE, "%s: the handle runs a fixed voice (synth_kind %u; sots_render_continuous renders it)", who, kind);
    if (feedback_genes)
        return fault(SOTS_ERR_STATE,
                     "%s: the feedback indices of operators 0x%x are genes (sots_create_graph_genes): every row has its own; sots_render_overlap_add "
                     "renders such a voice",
                     who, feedback_genes);
    return Fault{};
}

// sots_render_continuous: what it refuses before anything touches the device.  n, d, synth_arith: the context's audio
// length, genes per row and arithmetic mode.
inline Fault render_continuous_check(const sots_render_continuous_args *args, uint32_t n, uint32_t d, uint32_t synth_arith, const void *values,
                                     size_t values_bytes, uint32_t num_rows, const void *out, uint64_t out_samples)
{
    const char *who = "sots_render_continuous";
    if (const Fault f = render_cont_args_check(who, "sots_render_continuous_args", args, n)) return f;
    if (const Fault f = render_cont_track_check(who, args->hop, n, d, values, values_bytes, num_rows, out, out_samples)) return f;
    if (synth_arith == SOTS_ARITH_DEVICE_KERNELS)
        return fault(SOTS_ERR_STATE, "sots_render_continuous: not under SOTS_ARITH_DEVICE_KERNELS (that mode is the reference's kernels bit for bit)");
    return Fault{};
}

// ---- phase-continuous rendering of the operator-graph voice (sots_render_graph_continuous) ----
// level(j) = 0 for an unmodulated operator, else 1 + the largest level among its modulators: the operators of one level do
// not read each other and share three launches.  ops lists the operators by (level, j); level l holds ops[first[l]] ..
// ops[first[l + 1] - 1].  For a graph that voice_graph_check accepts.
struct GraphLevels {
    uint32_t count;                   // levels: 1 (a sum of unmodulated carriers) .. num_operators (a chain)
    uint32_t level_of[kGraphMaxOps];  // by operator
    uint32_t ops[kGraphMaxOps];       // operators, by (level, j)
    uint32_t first[kGraphMaxOps + 1]; // by level, into ops; first[count] = num_operators
};
inline GraphLevels graph_levels(const sots_voice_graph &g)
{
    GraphLevels l{};
    const uint32_t ops = g.num_operators < kGraphMaxOps ? g.num_operators : kGraphMaxOps;
    for (uint32_t j = 0; j < ops; ++j) {
        uint32_t lv = 0;
        for (uint32_t i = 0; i < j; ++i)
            if ((g.modulators[j] >> i & 1u) && l.level_of[i] + 1u > lv) lv = l.level_of[i] + 1u;
        l.level_of[j] = lv;
        if (lv + 1u > l.count) l.count = lv + 1u;
    }
    uint32_t filled = 0;
    for (uint32_t lv = 0; lv < l.count; ++lv) {
        l.first[lv] = filled;
        for (uint32_t j = 0; j < ops; ++j)
            if (l.level_of[j] == lv) l.ops[filled++] = j;
    }
    l.first[l.count] = filled;
    return l;
}
// whether reading operator i's output needs the wavetable: SQUARE and SAW are functions of the index alone
constexpr bool waveform_reads_table(uint32_t code) { return code != SOTS_WAVE_SQUARE && code != SOTS_WAVE_SAW; }
// whether the launches of level `level` read the table: some operator of the level has a modulator whose value is made from
// its phase word (it is not `flagged`: a feedback operator's shaped values are read as stored) by a shape that reads the table
inline bool graph_level_reads_table(const sots_voice_graph &g, const GraphLevels &l, const uint32_t codes[8], uint32_t level, uint32_t flagged = 0)
{
    for (uint32_t s = l.first[level]; s < l.first[level + 1u]; ++s)
        for (uint32_t i = 0; i < l.ops[s]; ++i)
            if ((g.modulators[l.ops[s]] >> i & 1u) && !(flagged >> i & 1u) && waveform_reads_table(codes[i])) return true;
    return false;
}
// Samples of a pass: a phase word per operator and sample and a shaped value per feedback operator and sample stay together
// within the 96 MiB that the fixed voices' renderer needs at the most (6 buffers of 2^22 words); whole tiles of 4096, at most
// 1024 of them (2^22 samples).
inline uint32_t graph_feedback_max_pass(uint32_t ops, uint32_t flagged)
{
    const uint32_t buffers = ops + flagged ? ops + flagged : 1u;
    const uint64_t tiles = (96ull << 20) / (sizeof(uint32_t) * buffers) / 4096u;
    return (uint32_t)(tiles < 1024u ? tiles : 1024u) * 4096u;
}
inline uint32_t graph_continuous_max_pass(uint32_t ops) { return graph_feedback_max_pass(ops, 0); }
// sots_render_graph_continuous: what it refuses before anything touches the device.  kind, feedback: the context's voice and
// its feedback indices; n, d: its audio length and genes per row.
inline Fault render_graph_continuous_check(uint32_t kind, const float feedback[8], const sots_render_continuous_args *args, uint32_t n, uint32_t d,
                                           const void *values, size_t values_bytes, uint32_t num_rows, const void *out, uint64_t out_samples,
                                           uint32_t feedback_genes = 0)
{
    const char *who = "sots_render_graph_continuous";
    if (const Fault f = render_graph_voice_check(who, kind, feedback_genes)) return f;
    for (uint32_t j = 0; j < kGraphMaxOps; ++j)
        if (feedback[j] != 0.0f)
            return fault(SOTS_ERR_STATE,
                         "sots_render_graph_continuous: operator %u has feedback index %g (sots_set_voice_feedback): a feedback operator's phase "
                         "offset is a serial recurrence that no scan computes; sots_render_overlap_add renders such a voice",
                         j, (double)feedback[j]);
    if (const Fault f = render_cont_args_check(who, "sots_render_continuous_args", args, n)) return f;
    return render_cont_track_check(who, args->hop, n, d, values, values_bytes, num_rows, out, out_samples);
}

// ---- ... with feedback operators (sots_render_graph_feedback) ----
// How a feedback operator's chain over the samples is computed (sots_render_graph_feedback_args.chain_form)
constexpr uint32_t kChainLibrary = 0, kChainSerial = 1, kChainRelax = 2;
constexpr uint32_t kRelaxCapMax = 4096, kRelaxCapLibrary = 1024;
// The library's choice of form for an operator of feedback index beta (!= 0), and of the cap.  The relaxation is chosen only
// for indices at which it beat the serial form in every repetition of the measurement of DESIGN.md 4.17
// (profiles/r27_render_graph_feedback.json): it did at 0.25, 0.5, 0.75, 1 and 1.5 (28 to 3.3 times faster) and did not at 2,
// where the chain is chaotic and a tile takes its thousand sweeps; nothing between 1.5 and 2 was measured.  The cap of 1024
// was the fastest or within a percent of it at every index.
constexpr float kRelaxBetaMax = 1.5f;
inline uint32_t graph_feedback_form(float beta) { return beta <= kRelaxBetaMax ? kChainRelax : kChainSerial; }
// What sots_render_graph_feedback and sots_render_graph_genes refuse alike before anything touches the device, under the name
// `who`: those of render_graph_continuous_check without the feedback one, and the two of their own arguments.
inline Fault render_graph_chain_check(const char *who, uint32_t kind, uint32_t feedback_genes, const sots_render_graph_feedback_args *args, uint32_t n,
                                      uint32_t d, const void *values, size_t values_bytes, uint32_t num_rows, const void *out, uint64_t out_samples)
{
    if (const Fault f = render_graph_voice_check(who, kind, feedback_genes)) return f;
    if (const Fault f = render_cont_args_check(who, "sots_render_graph_feedback_args", args, n)) return f;
    if (args->chain_form > kChainRelax)
        return fault(SOTS_ERR_INVALID, "%s: chain_form %u is not a form (0 = the library's choice, 1 = serial, 2 = relaxation)", who, args->chain_form);
    if (args->relax_cap > kRelaxCapMax) return fault(SOTS_ERR_INVALID, "%s: relax_cap %u outside 0..%u", who, args->relax_cap, kRelaxCapMax);
    return render_cont_track_check(who, args->hop, n, d, values, values_bytes, num_rows, out, out_samples);
}
// sots_render_graph_feedback: all of them, a context whose feedback indices are genes among them
inline Fault render_graph_feedback_check(uint32_t kind, const sots_render_graph_feedback_args *args, uint32_t n, uint32_t d, const void *values,
                                         size_t values_bytes, uint32_t num_rows, const void *out, uint64_t out_samples, uint32_t feedback_genes = 0)
{
    return render_graph_chain_check("sots_render_graph_feedback", kind, feedback_genes, args, n, d, values, values_bytes, num_rows, out, out_samples);
}

// ---- ... whose feedback indices are genes (sots_render_graph_genes) ----
// The operators whose chain a rendering runs ("flagged"): the gene operators, whatever their rows hold, and the others with
// beta_j != 0.  Per operator: whether it is flagged, whether its index is a gene, and the gene's column in a row of D.
struct GraphGeneOps {
    uint32_t flagged, genes;       // bit masks; genes is a subset of flagged
    uint32_t column[kGraphMaxOps]; // by operator; 0 where the operator's index is no gene
};
inline GraphGeneOps graph_gene_ops(uint32_t ops, uint32_t feedback_genes, const float feedback[8])
{
    GraphGeneOps g{};
    for (uint32_t j = 0; j < ops && j < kGraphMaxOps; ++j) {
        if (feedback_genes >> j & 1u) {
            g.genes |= 1u << j, g.flagged |= 1u << j;
            g.column[j] = feedback_gene_column(ops, feedback_genes, j);
        } else if (feedback[j] != 0.0f) {
            g.flagged |= 1u << j;
        }
    }
    return g;
}
// The form of a flagged operator's chain.  chain_form 1 and 2 force it.  Under the library's choice a fixed-index operator keeps
// graph_feedback_form(beta_j); a gene operator gets the relaxation (with the cap kRelaxCapLibrary where none is given),
// whatever its rows hold.  No rule on the rows is needed: in profiles/r27_render_graph_feedback.json the relaxation at cap 1024
// beat the serial form at every index up to 1.5, and at 2, where every tile takes its thousand sweeps, it cost what the
// serial form costs (311.5 against 310.3 ms).  Nothing between 1.5 and 2 was measured.  On a track whose index varies over
// [0, 2] from row to row the relaxation took 0.19 to 0.27 of the serial form's time (profiles/r31_render_graph_genes.json).
inline uint32_t graph_genes_form(uint32_t chain_form, bool gene, float beta)
{
    if (chain_form != kChainLibrary) return chain_form;
    return gene ? kChainRelax : graph_feedback_form(beta);
}
// sots_render_graph_genes: what it refuses before anything touches the device; those of render_graph_feedback_check under its
// own name, without the refusal of a gene mask.  d: the context's genes per row, 2 OPS + E.
inline Fault render_graph_genes_check(uint32_t kind, const sots_render_graph_feedback_args *args, uint32_t n, uint32_t d, const void *values,
                                      size_t values_bytes, uint32_t num_rows, const void *out, uint64_t out_samples)
{
    return render_graph_chain_check("sots_render_graph_genes", kind, 0, args, n, d, values, values_bytes, num_rows, out, out_samples);
}

// ---- time-parallel synthesis of the operator-graph voice (k_synth_graph_tp, sots_synth_graph_tp.hip) ----
// The PLAN of a checked graph: when each operator runs, how long its output is kept and where its buffers lie.  Computed
// here and nowhere else; the kernel receives the struct as an argument, so the host's capacity and the kernel's layout
// cannot disagree.
// The schedule, in ticks relative to a block's first: operator j SCANS the block at tick_of[j] (a modulated operator first
// forms its increments from its modulators' outputs) and EVALUATES it at tick_of[j] + 1, which makes its output o_j.
//   * tick_of[j] >= tick_of[i] + 2 for every modulator i of j (o_i is made strictly before j's scan reads it);
//   * the MIXER - the carrier with the latest tick, the largest j among equals - sums the carriers in the tick in which it
//     evaluates, so every other carrier runs at least one tick before it: tick_of[mixer] > tick_of[i];
//   * the first pass is as soon as possible, 2 x level (graph_levels) and one more for the mixer where another carrier shares
//     its level; the second, from the last operator down, as late as the readers allow, which shortens the rings.
// o_j of a block is read until tick last_read = max tick_of[its targets] (a modulator) or tick_of[mixer] + 1 (another
// carrier), so it needs a RING of depth[j] = last_read - tick_of[j] blocks: the block written depth[j] blocks later lands in
// the tick after the last read.  The mixer's own output stays in a register: depth 0.  Phases take two blocks per operator.
// An (individual, block) row is kGraphTpRow floats: 64 samples and 4 of padding, so that the scan's 16-byte accesses of
// neighbouring lanes fall on different banks (k_synth_tp's row).
constexpr uint32_t kGraphTpRow = 64 + 4;
constexpr uint32_t kGraphTpLdsBytes = 31 * 1024; // beside the 128 KiB table
struct GraphTpPlan {
    uint32_t ops, levels;
    uint32_t capacity;   // individuals per workgroup; 0: the graph's rows do not fit
    uint32_t rows;       // LDS rows per individual: 2 per operator (phases) + the ring depths
    uint32_t lag;        // ticks beyond the number of blocks: tick_of[mixer] + 1
    uint32_t mixer, num_carriers;
    uint32_t evaluators; // evaluating wavefronts per operator: 2 up to five operators, else 1 (at most 16 wavefronts)
    uint32_t tick_of[kGraphMaxOps], depth[kGraphMaxOps];
    uint32_t phase_off[kGraphMaxOps], ring_off[kGraphMaxOps]; // in floats, for `capacity` individuals per block
};
inline GraphTpPlan graph_tp_plan(const sots_voice_graph &g)
{
    GraphTpPlan p{};
    const GraphLevels lv = graph_levels(g);
    const uint32_t ops = g.num_operators < kGraphMaxOps ? g.num_operators : kGraphMaxOps;
    p.ops = ops;
    p.levels = lv.count;
    p.evaluators = ops <= 5u ? 2u : 1u;
    for (uint32_t j = 0; j < ops; ++j) {
        p.tick_of[j] = 2u * lv.level_of[j];
        if (g.carriers >> j & 1u) {
            ++p.num_carriers;
            if (p.num_carriers == 1u || p.tick_of[j] >= p.tick_of[p.mixer]) p.mixer = j;
        }
    }
    for (uint32_t j = 0; j < ops; ++j)
        if ((g.carriers >> j & 1u) && j != p.mixer && p.tick_of[j] == p.tick_of[p.mixer]) {
            ++p.tick_of[p.mixer];
            break;
        }
    // as late as the readers allow, from the last operator down (a reader has a larger index, or is the mixer)
    for (uint32_t j = ops; j-- > 0;) {
        if (j == p.mixer) continue;
        uint32_t latest = ~0u;
        if (g.carriers >> j & 1u) latest = p.tick_of[p.mixer] - 1u;
        for (uint32_t k = j + 1; k < ops; ++k)
            if ((g.modulators[k] >> j & 1u) && p.tick_of[k] - 2u < latest) latest = p.tick_of[k] - 2u;
        if (latest != ~0u && latest > p.tick_of[j]) p.tick_of[j] = latest;
    }
    p.lag = p.tick_of[p.mixer] + 1u;
    p.rows = 2u * ops;
    for (uint32_t j = 0; j < ops; ++j) {
        if (j == p.mixer) continue;
        uint32_t last_read = 0;
        if (g.carriers >> j & 1u) last_read = p.tick_of[p.mixer] + 1u;
        for (uint32_t k = j + 1; k < ops; ++k)
            if ((g.modulators[k] >> j & 1u) && p.tick_of[k] > last_read) last_read = p.tick_of[k];
        p.depth[j] = last_read > p.tick_of[j] ? last_read - p.tick_of[j] : 0u;
        p.rows += p.depth[j];
    }
    p.capacity = kGraphTpLdsBytes / (p.rows * kGraphTpRow * (uint32_t)sizeof(float));
    if (p.capacity > 64u) p.capacity = 64u; // (a lane per individual in the scans)
    uint32_t at = 0;
    for (uint32_t j = 0; j < ops; ++j) {
        p.phase_off[j] = at;
        at += 2u * p.capacity * kGraphTpRow;
        p.ring_off[j] = at;
        at += p.depth[j] * p.capacity * kGraphTpRow;
    }
    return p;
}
// LDS bytes of a plan's buffers (<= kGraphTpLdsBytes)
inline uint32_t graph_tp_bytes(const GraphTpPlan &p) { return p.rows * p.capacity * kGraphTpRow * (uint32_t)sizeof(float); }

// Where AUTO takes the time-parallel form: a CU's share of the rows of at most this many individuals, by operator count
// (index OPS; 0: never).  From profiles/r33_graph_time_parallel.json, one job on one MI355X, the two forms alternating over
// three rounds on one context: the largest share up to which the form beat the lane form in every round by more than the lane
// leg's own round-to-round spread, in synthesis launch time and per generation, at N = 1024 and 2048 and at every measured
// share below it.  For the operator counts measured it did at every share that fits one group - the entries are the
// capacities of 2op (19), chain3 and two_mods (11), fan3 (8) and triple (5) - and nowhere near: the closest leg is 2op at a
// share of 19 and N = 1024, 67 against 103 us per launch with a lane spread below 1.  A graph that holds
// fewer than its count's entry stops at its own capacity.  Graphs of 5, 7 and 8 operators were NOT measured: AUTO keeps the
// lane form for them until they are.
constexpr uint32_t kGraphTpAutoShare[kGraphMaxOps + 1] = {0, 0, 19, 11, 8, 0, 5, 0, 0};
// The form that a synthesis of `rows` rows launches (SOTS_GRAPH_FORM_LANES or SOTS_GRAPH_FORM_TIME_PARALLEL): read by the
// launcher and by the getters.  Feedback - an index other than 0 or a gene mask - and a graph whose plan holds nobody keep
// the lane form whatever is requested; a forced TIME_PARALLEL takes any number of rows (in several groups per CU where the
// share exceeds the capacity); AUTO takes it where the share fits one group and is at most the measured limit.
inline uint32_t graph_synth_form_for(uint32_t requested, const sots_voice_graph &g, const float *feedback, uint32_t feedback_genes, uint64_t rows,
                                     uint32_t num_cus)
{
    if (requested == SOTS_GRAPH_FORM_LANES || feedback_genes) return SOTS_GRAPH_FORM_LANES;
    if (feedback)
        for (uint32_t j = 0; j < kGraphMaxOps && j < g.num_operators; ++j)
            if (feedback[j] != 0.0f) return SOTS_GRAPH_FORM_LANES;
    const GraphTpPlan p = graph_tp_plan(g);
    if (p.capacity == 0) return SOTS_GRAPH_FORM_LANES;
    if (requested == SOTS_GRAPH_FORM_TIME_PARALLEL) return SOTS_GRAPH_FORM_TIME_PARALLEL;
    const uint32_t cus = num_cus ? num_cus : 256u;
    const uint64_t share = (rows + cus - 1u) / cus;
    return share <= p.capacity && share <= kGraphTpAutoShare[p.ops] ? SOTS_GRAPH_FORM_TIME_PARALLEL : SOTS_GRAPH_FORM_LANES;
}
// sots_set_graph_synth_form / sots_get_graph_synth_form: a fixed voice has no forms; an unknown code
inline Fault graph_synth_form_check(uint32_t kind, uint32_t form)
{
    if (kind != SOTS_SYNTH_GRAPH) return fault(SOTS_ERR_STATE, "graph synthesis form: the handle runs a fixed voice (synth_kind %u)", kind);
    if (form > SOTS_GRAPH_FORM_TIME_PARALLEL)
        return fault(SOTS_ERR_INVALID, "graph synthesis form: %u is not a form (0 = auto, 1 = lanes, 2 = time-parallel)", form);
    return Fault{};
}

// ---- run record, stop rules ----
constexpr uint64_t kTrackMaxRecords = 1ull << 24; // chunks x history_capacity (1.5 GiB of records)
// sots_track / sots_batch_track: known flags, a history with a period and room, and no more than kTrackMaxRecords records
// over the handle's chunks.  *flags comes back normalised (HISTORY implies BEST_EVER).  max_chunks 0: a context, one
// population whose refusal has no chunk count to name.
inline Fault track_args_check(uint32_t *flags, uint32_t history_every, uint32_t history_capacity, uint32_t max_chunks)
{
    if (*flags & ~(uint32_t)(SOTS_TRACK_BEST_EVER | SOTS_TRACK_HISTORY)) return fault(SOTS_ERR_INVALID, "unknown track flags %u", *flags);
    if (!(*flags & SOTS_TRACK_HISTORY)) return Fault{};
    *flags |= SOTS_TRACK_BEST_EVER;
    if (history_every == 0 || history_capacity == 0)
        return fault(SOTS_ERR_INVALID, "history needs history_every >= 1 and history_capacity >= 1 (got %u, %u)", history_every, history_capacity);
    if (max_chunks == 0 && history_capacity > kTrackMaxRecords)
        return fault(SOTS_ERR_INVALID, "history_capacity %u exceeds %llu records", history_capacity, (unsigned long long)kTrackMaxRecords);
    if ((uint64_t)history_capacity * max_chunks > kTrackMaxRecords)
        return fault(SOTS_ERR_INVALID, "history_capacity %u x max_chunks %u exceeds %llu records", history_capacity, max_chunks,
                     (unsigned long long)kTrackMaxRecords);
    return Fault{};
}

inline int stop_rule_check(const sots_stop_rule *rule)
{
    if (!rule || rule->struct_size != sizeof(sots_stop_rule) || rule->check_interval == 0) return SOTS_ERR_INVALID;
    return SOTS_OK;
}

// ---- chunk queue: carried rows (sots_batch_queue_set_carry) ----
// rows 0 turns carrying off (the segment length is then ignored); otherwise 1 <= rows <= numParents - recombination reads
// parent rows only - and segments of at least one chunk
inline Fault queue_carry_check(uint32_t rows, uint32_t segment, uint32_t num_parents)
{
    if (rows == 0) return Fault{};
    if (rows > num_parents)
        return fault(SOTS_ERR_INVALID, "sots_batch_queue_set_carry: %u carried rows asked for, at most numParents = %u can be carried", rows, num_parents);
    if (segment == 0) return fault(SOTS_ERR_INVALID, "sots_batch_queue_set_carry: segment_chunks must be at least 1 with carry_rows %u", rows);
    return Fault{};
}

// How a run of `chunks` (>= 1) queued chunks is laid out over a handle of max_chunks (>= 1) slots.  Without carrying
// (rows 0) every chunk is a segment of its own: segment 1, segments = chunks.  With it a segment never holds more than
// the whole queue, so the length counts as min(segment, chunks).  Slot c starts with chunk c * segment.
struct QueuePlan {
    uint32_t segment, segments, slots;
};
inline QueuePlan queue_plan(uint32_t chunks, uint32_t max_chunks, uint32_t carry_rows, uint32_t segment_chunks)
{
    QueuePlan p;
    p.segment = carry_rows == 0 ? 1u : (segment_chunks < chunks ? segment_chunks : chunks);
    p.segments = (chunks - 1u) / p.segment + 1u;
    p.slots = p.segments < max_chunks ? p.segments : max_chunks;
    return p;
}

// Loop generations within which the last chunk retires.  No chunk runs longer than max_generations, so no segment runs
// longer than segment * max_generations.  Without a rule every segment but the last takes exactly that and the slots turn
// over together: ceil(segments / slots) rounds.  With a rule a slot draws its last segment no later than
// (segments - 1) / slots + 1 full rounds after the start and needs one more to end it.  Saturates at UINT64_MAX.
inline uint64_t queue_loop_bound(const QueuePlan &p, uint32_t max_generations, bool with_rule)
{
    const uint64_t rounds = with_rule ? (uint64_t)(p.segments - 1u) / p.slots + 2u : ((uint64_t)p.segments + p.slots - 1u) / p.slots;
    const uint64_t per_round = (uint64_t)p.segment * max_generations; // < 2^64
    if (per_round != 0 && rounds > ~0ull / per_round) return ~0ull;
    return rounds * per_round;
}

} // namespace sots
