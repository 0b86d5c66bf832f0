// sots_synth_graph.hip -- the operator-graph voice (SOTS_SYNTH_GRAPH): one synthesis kernel for every feed-forward FM
// algorithm of 2 to 8 operators.  The voice is defined in include/sots_hip.h (sots_voice_graph); this file follows that
// definition operation by operation, unfused (-ffp-contract=off), so the audio equals the serial model bit for bit.
//
// Shape, after k_synth<K, 0> (sots_kernels.hip): a lane per individual, the 128 KiB wavetable staged into LDS once per
// persistent workgroup (one workgroup per CU), finished samples parked in a per-wavefront swizzled LDS tile and stored as
// whole lines of a row.  What differs:
//   * the topology is an ARGUMENT: the masks arrive as kernel arguments (scalar registers), and every test on them is
//     wavefront-uniform.  The loops over operators j and modulators i < j are unrolled with compile-time indices, so
//     phases, frequencies and levels stay in registers;
//   * no software pipeline across loop trips and no cut forms: samples go in blocks of U, operator by operator inside a
//     block, so that an operator's U table reads are in flight together and waited for once (sample by sample, each read
//     is waited for where it is used: 117 us for the 2-op graph at P = 65 536 against 99 in blocks).
// A cleared bit is SKIPPED, as the definition says: a sum starts from -0.0f, for which -0 + x == x bit for bit for every
// x (+0 and -0 included), and only operators whose bit is set are added to it.
#include "kernels/common.h"
#include <cstdlib>
#include <type_traits>

#pragma clang fp contract(off)
namespace sots {
namespace {

struct GraphMasks {
    uint32_t carriers;
    uint32_t modulators[8];
};
struct GraphFeedback {
    float b[8]; // beta_j K
};
constexpr uint32_t kGeneShift = 24; // the gene form's codes word: operator j's code in bits 3j..3j+2, its mask bit at 24 + j
// Feedback indices as genes (sots_create_graph_genes): which operators, the floats between rows of `values`, and per gene
// operator its column and that column's range (the entries of SynthParams the column number would pick: an operator
// number known at compile time picks them here, so nothing is indexed by a run-time value)
struct GraphGenes {
    uint32_t mask, stride;
    uint32_t col[8];
    float pmin[8], pmax[8];
};
template <typename T, typename... R>
__device__ __forceinline__ T first_of(T first, R...)
{
    return first;
}
template <typename T, typename S, typename... R>
__device__ __forceinline__ S second_of(T, S second, R...)
{
    return second;
}

// The operators' waveforms (sots_set_voice_waveforms, include/sots_hip.h).  SHAPES is empty or one uint32_t: the kernel
// with no such argument is the all-sine voice with the arguments it always had; with it, every operator's table value goes
// through shape(w_j, i) before its level multiplies it.  The argument holds the codes, 3 bits per operator, in a scalar
// register, and an operator's block of U reads runs under a wavefront-uniform branch on its code: each shape is its own
// straight-line statement of the definition, decided on the integer index, and SQUARE and SAW read no table at all.
// (The form that lost, DESIGN.md 4.14: one branchless body with per-operator scalar constants - index shift, sign mask,
// zeroing index bit, two overrides - costs every code the instructions of all of them.)
// Feedback (sots_set_voice_feedback, include/sots_hip.h): SHAPES is the codes and GraphFeedback, the eight
// B_j = beta_j K as scalar arguments.  An operator with B_j != 0 (wavefront-uniform) reads the table at its phase offset by
// B_j times the mean of its own last two shaped values: its block of U reads is a serial chain offset -> wraps -> index ->
// read -> next offset, so its U phases are advanced first (they do not depend on the feedback) and the chain runs after
// them.  h1 and h2 stay in registers across blocks, flushes and tiles and are reset per row.  An operator with B_j == 0
// runs the shaped form's block as it stands.
// Feedback genes (sots_create_graph_genes, include/sots_hip.h): SHAPES is the codes, GraphGenes and
// GraphFeedback (the codes stay first and the indices last, where the feedback form looks for them).  Rows of `values` are
// genes.stride floats apart.  An operator whose mask bit is set (wavefront-uniform) has B_j in a register per lane, made
// once per row from its gene - scaled, clamped to the effective index, times K - and ALWAYS runs the chain, also in lanes
// where B_j is +0; every other operator takes the two paths of the feedback form, its B_j the scalar argument.  The chain
// is written out once for each: the feedback form's own lines stay as they are, so its code objects do too.
// CH: 16-byte chunks per tile row = 4 CH samples per flush.  The 32 KiB beside the table are 32 / CH tiles of 64 rows:
// CH = 8, four wavefronts (one per SIMD) and whole 128-byte lines; CH = 4, eight wavefronts (two per SIMD) and half lines.
template <int OPS, int CH, typename... SHAPES>
__global__ __launch_bounds__((32 / CH) * kWave) void k_synth_graph(const float *__restrict__ values, const float *__restrict__ wavetable,
                                                                  float *__restrict__ audio, SynthParams sp, GraphMasks gm, uint32_t p_len,
                                                                  uint32_t n, uint32_t pitch, SHAPES... shapes)
{
    constexpr bool SHAPED = sizeof...(SHAPES) != 0;
    // (an experiment build also has the form that lost: the codes as int32_t)
    constexpr bool BRANCHES = SHAPED && (std::is_same_v<SHAPES, uint32_t> || ...);
    constexpr bool FEEDBACK = (std::is_same_v<SHAPES, GraphFeedback> || ...);
    constexpr bool GENES = (std::is_same_v<SHAPES, GraphGenes> || ...);
    static_assert((sizeof...(SHAPES) <= 1 && ((std::is_same_v<SHAPES, uint32_t> || std::is_same_v<SHAPES, int32_t>) && ...)) ||
                      (sizeof...(SHAPES) == 2 && BRANCHES && FEEDBACK && !GENES) || (sizeof...(SHAPES) == 3 && BRANCHES && FEEDBACK && GENES),
                  "no argument, the packed codes, the packed codes and the feedback indices, or those and the feedback genes");
    constexpr int D = 2 * OPS, WAVES = 32 / CH; // (D: the genes of the forms without feedback genes)
    constexpr int RPI = kWave / CH; // rows per transposed read / store instruction (CH of them per flush)
    constexpr int U = OPS <= 4 ? 8 : 4;            // samples per block: o[OPS][U] stays in registers
    constexpr int kUnroll = OPS <= 2 && !FEEDBACK ? CH / (U / 4) : 1; // blocks unrolled per flush: the code stays in the instruction cache
    static_assert(U % 4 == 0 && CH % (U / 4) == 0, "whole 16-byte chunks, whole blocks per flush");
    static_assert(OPS >= 2 && OPS <= 8 && D <= SOTS_MAX_DIMS && (CH == 8 || CH == 4), "2 to 8 operators; whole or half lines");
    __shared__ float tab[kWavetableSize];
    __shared__ float4 stage_all[WAVES * kWave * CH];
    request_wavetable(tab, wavetable);
    const float wf = (float)kWavetableSize;
    const float c = (float)kWavetableSize / (float)SOTS_SAMPLE_RATE;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    // the tile (k_synth's): lane = row on the write side, chunk q of a row in slot q ^ swz(row); on the read side lane =
    // (row within a group of RPI rows, chunk), and group g lies 64 slots further
    float4 *stage = stage_all + wave * kWave * CH;
    auto swz = [](uint32_t row) { return CH == 8 ? (row & 7u) : ((row >> 1) & 3u); };
    float4 *wr = stage + lane * CH;
    const uint32_t l7 = swz(lane);
    const uint32_t r8 = lane / CH, rch = lane % CH;
    const float4 *rd = stage + r8 * CH + (rch ^ swz(r8));

    // table[clamp((int)pos, 0, W-1)], the clamp decided on the float: NaN and negatives give entry 0
    auto index_of = [&](float pos) { return (uint32_t)fminf(fmaxf(pos, 0.0f), wf - 1.0f); };
    auto tab_at = [&](float pos) { return tab[index_of(pos)]; };
    uint32_t num_carriers = 0;
#pragma unroll
    for (int j = 0; j < OPS; ++j) num_carriers += gm.carriers >> j & 1u;
    const float carriers_f = (float)num_carriers;

    wavetable_ready();
    const uint32_t rows_per_block = blockDim.x; // a row per lane
    for (uint32_t base = blockIdx.x * rows_per_block; base < p_len; base += gridDim.x * rows_per_block) {
        const uint32_t row0 = base + wave * kWave; // first row of this wavefront
        if (row0 >= p_len) continue;               // (wavefront-uniform; no workgroup barrier below)
        const uint32_t ind = row0 + lane < p_len ? row0 + lane : p_len - 1u;
        float f[OPS], amp[OPS], pos[OPS];
        [[maybe_unused]] float h1[OPS], h2[OPS]; // (feedback: an operator's last two shaped values, +0 at sample 0)
        [[maybe_unused]] float bg[OPS];          // (feedback genes: a gene operator's B_j of this lane's row)
        uint32_t stride = (uint32_t)D;           // floats between rows of values
        if constexpr (GENES) {
            const GraphGenes gg = second_of(shapes...);
            stride = gg.stride;
#pragma unroll
            for (int j = 0; j < OPS; ++j) {
                bg[j] = 0.0f;
                if (gg.mask >> j & 1u) { // beta = p > 0 ? fminf(p, 2) : +0 (NaN and negatives: +0); B = beta K
                    const float p = gg.pmin[j] + values[(size_t)ind * stride + gg.col[j]] * (gg.pmax[j] - gg.pmin[j]);
                    bg[j] = (p > 0.0f ? fminf(p, 2.0f) : 0.0f) * kFeedbackScale;
                }
            }
        }
        if constexpr (FEEDBACK) {
#pragma unroll
            for (int j = 0; j < OPS; ++j) h1[j] = h2[j] = 0.0f;
        }
#pragma unroll
        for (int j = 0; j < OPS; ++j) {
            const float a = sp.pmin[2 * j + 1] + values[(size_t)ind * stride + 2 * j + 1] * (sp.pmax[2 * j + 1] - sp.pmin[2 * j + 1]);
            f[j] = sp.pmin[2 * j] + values[(size_t)ind * stride + 2 * j] * (sp.pmax[2 * j] - sp.pmin[2 * j]);
            amp[j] = (gm.carriers >> j & 1u) ? a : f[j] * a;
            pos[j] = 0.0f;
        }
        // U samples at a time, operator by operator: operator j's sample u needs its own phase and the outputs o[i][u] of
        // the operators i < j, which the block already holds - the order of the definition, sample by sample, is kept for
        // every value.  An operator's U table reads are issued with nothing but its phase recurrence between them and
        // waited for once, before its outputs are made.
        auto block = [&](float(&y)[U]) {
            float o[OPS][U];
            static_for<0, OPS>([&](auto j_tag) {
                constexpr int J = decltype(j_tag)::value;
                float cur[U], tv[U];
#pragma unroll
                for (int u = 0; u < U; ++u) cur[u] = -0.0f;
                static_for<0, J>([&](auto i_tag) {
                    constexpr int I = decltype(i_tag)::value;
                    if (gm.modulators[J] >> I & 1u) {
#pragma unroll
                        for (int u = 0; u < U; ++u) cur[u] += o[I][u];
                    }
                });
                const bool modulated = gm.modulators[J] != 0u;
                if constexpr (BRANCHES) {
                    // (the code is taken from the argument here, block by block: the tests on it held in scalar registers
                    // across the sample loop for every operator cost the wide forms register lanes)
                    uint32_t packed = first_of(shapes...);
                    asm volatile("" : "+s"(packed));
                    const uint32_t w = packed >> (3 * J) & 7u;
                    [[maybe_unused]] uint32_t fb_bits = 0u; // B_J's bits: checked indices are +0 or positive, so 0 is "off"
                    if constexpr (FEEDBACK) {
                        fb_bits = __float_as_uint((shapes, ...).b[J]);
                        asm volatile("" : "+s"(fb_bits));
                    }
                    auto run = [&](auto shape) {
                        if constexpr (FEEDBACK) {
                            if constexpr (GENES) {
                                // (the mask rides in bits 24..31 of the codes' word, above the eight 3-bit codes: the word the
                                // block fetches anyway says which path the operator takes.  Measured against it, DESIGN.md 4.18:
                                // the mask as a scalar of its own (the same), a marker among the scalar B_J (slower) and ONE chain
                                // for both kinds of operator with the scalar B_J copied into a register (slower))
                                // (this chain is a copy of the fixed index's below: keep the two identical but for bj)
                                if (packed >> (kGeneShift + J) & 1u) { // a gene operator always runs the chain, whatever its lanes' B_J
                                    const float bj = bg[J];
                                    float ph[U];
#pragma unroll
                                    for (int u = 0; u < U; ++u) {
                                        ph[u] = pos[J];
                                        pos[J] += c * (cur[u] + f[J]);
                                        if (pos[J] >= wf) pos[J] -= wf;
                                        if (modulated && pos[J] < 0.0f) pos[J] += wf;
                                    }
                                    float a1 = h1[J], a2 = h2[J];
#pragma unroll
                                    for (int u = 0; u < U; ++u) {
                                        const float g = (a1 + a2) * 0.5f;
                                        float z = ph[u] + bj * g;
                                        if (z >= wf) z -= wf;
                                        if (z < 0.0f) z += wf;
                                        tv[u] = shape(index_of(z));
                                        a2 = a1;
                                        a1 = tv[u];
                                    }
                                    h1[J] = a1;
                                    h2[J] = a2;
                                    return;
                                }
                            }
                            // (the chain of the fixed index: keep it the gene copy above, statement for statement - only bj's
                            // source differs)
                            if (fb_bits != 0u) {
                                const float bj = __uint_as_float(fb_bits);
                                float ph[U];
#pragma unroll
                                for (int u = 0; u < U; ++u) {
                                    ph[u] = pos[J];
                                    pos[J] += c * (cur[u] + f[J]);
                                    if (pos[J] >= wf) pos[J] -= wf;
                                    if (modulated && pos[J] < 0.0f) pos[J] += wf;
                                }
                                float a1 = h1[J], a2 = h2[J];
#pragma unroll
                                for (int u = 0; u < U; ++u) {
                                    const float g = (a1 + a2) * 0.5f;
                                    float z = ph[u] + bj * g;
                                    if (z >= wf) z -= wf;
                                    if (z < 0.0f) z += wf;
                                    tv[u] = shape(index_of(z));
                                    a2 = a1;
                                    a1 = tv[u];
                                }
                                h1[J] = a1;
                                h2[J] = a2;
                                return;
                            }
                        }
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            tv[u] = shape(index_of(pos[J]));
                            pos[J] += c * (cur[u] + f[J]);
                            if (pos[J] >= wf) pos[J] -= wf;
                            if (modulated && pos[J] < 0.0f) pos[J] += wf;
                        }
                    };
                    constexpr uint32_t H = (uint32_t)kWavetableSize / 2u, Q = (uint32_t)kWavetableSize / 4u;
                    switch (w) {
                    case SOTS_WAVE_HALF: run([&](uint32_t i) { return i < H ? tab[i] : 0.0f; }); break;
                    case SOTS_WAVE_ABS: run([&](uint32_t i) { return fabsf(tab[i]); }); break;
                    case SOTS_WAVE_PULSE: run([&](uint32_t i) { return (i & Q) == 0 ? fabsf(tab[i]) : 0.0f; }); break;
                    case SOTS_WAVE_EVEN: run([&](uint32_t i) { return i < H ? tab[2u * i] : 0.0f; }); break;
                    case SOTS_WAVE_ABS_EVEN: run([&](uint32_t i) { return i < H ? fabsf(tab[2u * i]) : 0.0f; }); break;
                    case SOTS_WAVE_SQUARE: run([&](uint32_t i) { return i < H ? 1.0f : -1.0f; }); break;
                    case SOTS_WAVE_SAW: run([&](uint32_t i) { return (float)i * 0x1p-14f - 1.0f; }); break;
                    default: run([&](uint32_t i) { return tab[i]; }); break;
                    }
                } else if constexpr (SHAPED) {
                    // (the constants are derived here, block by block: held across the sample loop for every operator they
                    // cost the 7-operator form 36 bytes of scratch)
                    uint32_t packed = (uint32_t)(shapes, ...);
                    asm volatile("" : "+s"(packed));
                    const uint32_t w = packed >> (3 * J) & 7u;
                    const uint32_t shift = (w == SOTS_WAVE_EVEN || w == SOTS_WAVE_ABS_EVEN) ? 1u : 0u;
                    const uint32_t keep = (w == SOTS_WAVE_ABS || w == SOTS_WAVE_PULSE || w == SOTS_WAVE_ABS_EVEN) ? 0x7fffffffu : 0xffffffffu;
                    const uint32_t zero_at = w == SOTS_WAVE_PULSE ? (uint32_t)kWavetableSize / 4u
                                             : (w == SOTS_WAVE_HALF || w == SOTS_WAVE_EVEN || w == SOTS_WAVE_ABS_EVEN) ? (uint32_t)kWavetableSize / 2u : 0u;
                    uint32_t at[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        at[u] = index_of(pos[J]);
                        tv[u] = tab[(at[u] << shift) & ((uint32_t)kWavetableSize - 1u)]; // (inside the table whatever the code)
                        pos[J] += c * (cur[u] + f[J]);
                        if (pos[J] >= wf) pos[J] -= wf;
                        if (modulated && pos[J] < 0.0f) pos[J] += wf;
                    }
                    if (w == SOTS_WAVE_SQUARE) {
#pragma unroll
                        for (int u = 0; u < U; ++u) tv[u] = at[u] < (uint32_t)kWavetableSize / 2u ? 1.0f : -1.0f;
                    } else if (w == SOTS_WAVE_SAW) {
#pragma unroll
                        for (int u = 0; u < U; ++u) tv[u] = (float)at[u] * 0x1p-14f - 1.0f; // (both exact below 2^15)
                    } else {
#pragma unroll
                        for (int u = 0; u < U; ++u) tv[u] = (at[u] & zero_at) ? 0.0f : __uint_as_float(__float_as_uint(tv[u]) & keep);
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        tv[u] = tab_at(pos[J]);
                        pos[J] += c * (cur[u] + f[J]);
                        if (pos[J] >= wf) pos[J] -= wf;
                        if (modulated && pos[J] < 0.0f) pos[J] += wf;
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) o[J][u] = tv[u] * amp[J];
            });
#pragma unroll
            for (int u = 0; u < U; ++u) y[u] = -0.0f;
            static_for<0, OPS>([&](auto j_tag) {
                constexpr int J = decltype(j_tag)::value;
                if (gm.carriers >> J & 1u) {
#pragma unroll
                    for (int u = 0; u < U; ++u) y[u] += o[J][u];
                }
            });
            if (num_carriers > 1u) {
#pragma unroll
                for (int u = 0; u < U; ++u) y[u] = y[u] / carriers_f;
            }
        };
        for (uint32_t i0 = 0; i0 < n; i0 += 4u * CH) {
#pragma unroll kUnroll
            for (uint32_t q = 0; q < (uint32_t)CH; q += U / 4) {
                float y[U];
                block(y);
#pragma unroll
                for (int k = 0; k < U / 4; ++k) wr[(q + k) ^ l7] = make_float4(y[4 * k], y[4 * k + 1], y[4 * k + 2], y[4 * k + 3]);
            }
            // 4 CH samples of 64 rows are parked: read back transposed, RPI rows x whole (half) lines per store
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
#pragma unroll 4 // (four lines in flight: all eight at once cost the 8-operator form its 128 registers)
            for (uint32_t g = 0; g < (uint32_t)CH; ++g) {
                const uint32_t row = row0 + g * RPI + r8;
                if (row < p_len) *reinterpret_cast<float4 *>(audio + (size_t)row * pitch + i0 + 4u * rch) = rd[g * kWave];
            }
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
        }
    }
}

template <int OPS>
hipError_t launch_ops(hipStream_t st, const GraphMasks &gm, const float *values, const float *wavetable, float *audio, const SynthParams &sp,
                      uint32_t p, uint32_t n, uint32_t pitch, uint32_t cus, uint32_t shapes, const GraphFeedback *fb, const GraphGenes *genes)
{
    // one workgroup per CU (the table), sized to the CU's share of the population up to one wavefront per SIMD; larger
    // populations loop over tiles
    uint32_t max_waves = 4;
#ifdef SOTS_EXPERIMENT
    if (const char *e = getenv("SOTS_GRAPH_WAVES")) max_waves = atoi(e) == 8 ? 8 : 4; // 8: two per SIMD, half-line tiles
#endif
    const uint32_t share = (p + cus - 1) / cus;
    uint32_t waves = (share + kWave - 1) / kWave;
    if (waves > max_waves) waves = max_waves;
    if ((shapes || fb || genes) && waves > 4) waves = 4; // (the CH = 4 experiment form is not shaped)
    const uint32_t rows = waves * kWave, tiles = (p + rows - 1) / rows, grid = tiles < cus ? tiles : cus;
    if (genes) { // any operator's index is a gene: the codes and the fixed indices (all +0 without any) go through this form too
        k_synth_graph<OPS, 8, uint32_t, GraphGenes, GraphFeedback>
            <<<grid, rows, 0, st>>>(values, wavetable, audio, sp, gm, p, n, pitch, shapes | genes->mask << kGeneShift, *genes, fb ? *fb : GraphFeedback{});
        return hipGetLastError();
    }
    if (fb) { // any operator feeds back: the codes go through this form too (all sine through the switch's default)
        k_synth_graph<OPS, 8, uint32_t, GraphFeedback><<<grid, rows, 0, st>>>(values, wavetable, audio, sp, gm, p, n, pitch, shapes, *fb);
        return hipGetLastError();
    }
#ifdef SOTS_EXPERIMENT
    if (const char *e = getenv("SOTS_GRAPH_SHAPE_CONSTANTS"); shapes && e && atoi(e) == 1) {
        k_synth_graph<OPS, 8, int32_t><<<grid, rows, 0, st>>>(values, wavetable, audio, sp, gm, p, n, pitch, (int32_t)shapes);
        return hipGetLastError();
    }
#endif
    if (shapes) { // any setting but all sine
        k_synth_graph<OPS, 8, uint32_t><<<grid, rows, 0, st>>>(values, wavetable, audio, sp, gm, p, n, pitch, shapes);
        return hipGetLastError();
    }
#ifdef SOTS_EXPERIMENT
    if (max_waves == 8) {
        k_synth_graph<OPS, 4><<<grid, rows, 0, st>>>(values, wavetable, audio, sp, gm, p, n, pitch);
        return hipGetLastError();
    }
#endif
    k_synth_graph<OPS, 8><<<grid, rows, 0, st>>>(values, wavetable, audio, sp, gm, p, n, pitch);
    return hipGetLastError();
}

} // namespace

hipError_t launch_synth_graph(hipStream_t st, const sots_voice_graph &graph, const float *values, const float *wavetable, float *audio,
                              const SynthParams &sp, uint32_t p, uint32_t log2n, uint32_t pitch, uint32_t num_cus, uint32_t waveforms,
                              const float *feedback, uint32_t feedback_genes, uint32_t form)
{
    if (p == 0 || log2n < 8 || pitch < (1u << log2n) || pitch % 4u != 0) return hipErrorInvalidValue; // (a flush is 32 samples; 16-byte stores)
    // the time axis in the lanes (k_synth_graph_tp, sots_synth_graph_tp.hip) where the rule gives these rows to it
    if (graph_synth_form_for(form, graph, feedback, feedback_genes, p, num_cus) == SOTS_GRAPH_FORM_TIME_PARALLEL)
        return launch_synth_graph_tp(st, graph, values, wavetable, audio, sp, p, log2n, pitch, num_cus, waveforms);
    GraphMasks gm;
    gm.carriers = graph.carriers;
    for (int j = 0; j < 8; ++j) gm.modulators[j] = graph.modulators[j];
    const uint32_t n = 1u << log2n, cus = num_cus ? num_cus : 256;
    // (checked codes hold nothing beyond the operators: all sine is 0 and launches the kernel without the argument)
    const uint32_t shapes = graph.num_operators < 8 ? waveforms & ((1u << 3 * graph.num_operators) - 1u) : waveforms & 0xFFFFFFu;
    // (checked indices are +0 beyond the operators; all zero launches what is launched without the setting)
    GraphFeedback scaled;
    const GraphFeedback *fb = feedback && scale_feedback(feedback, graph.num_operators, scaled.b) ? &scaled : nullptr;
    // (a checked mask holds nothing beyond the operators; 0 launches what is launched without it)
    GraphGenes held{};
    const GraphGenes *genes = nullptr;
    if (const uint32_t mask = feedback_genes & ((1u << graph.num_operators) - 1u)) {
        held.mask = mask;
        held.stride = graph_dims(graph.num_operators, mask);
        if (held.stride > SOTS_MAX_DIMS) return hipErrorInvalidValue;
        for (uint32_t j = 0; j < graph.num_operators; ++j) {
            if (!(mask >> j & 1u)) continue;
            held.col[j] = feedback_gene_column(graph.num_operators, mask, j);
            held.pmin[j] = sp.pmin[held.col[j]];
            held.pmax[j] = sp.pmax[held.col[j]];
        }
        genes = &held;
    }
    switch (graph.num_operators) {
    case 2: return launch_ops<2>(st, gm, values, wavetable, audio, sp, p, n, pitch, cus, shapes, fb, genes);
    case 3: return launch_ops<3>(st, gm, values, wavetable, audio, sp, p, n, pitch, cus, shapes, fb, genes);
    case 4: return launch_ops<4>(st, gm, values, wavetable, audio, sp, p, n, pitch, cus, shapes, fb, genes);
    case 5: return launch_ops<5>(st, gm, values, wavetable, audio, sp, p, n, pitch, cus, shapes, fb, genes);
    case 6: return launch_ops<6>(st, gm, values, wavetable, audio, sp, p, n, pitch, cus, shapes, fb, genes);
    case 7: return launch_ops<7>(st, gm, values, wavetable, audio, sp, p, n, pitch, cus, shapes, fb, genes);
    case 8: return launch_ops<8>(st, gm, values, wavetable, audio, sp, p, n, pitch, cus, shapes, fb, genes);
    default: return hipErrorInvalidValue;
    }
}

} // namespace sots
