// sots_render.h -- overlap-add resynthesis of a parameter track (sots_render.hip) and its phase-continuous
// rendering (sots_render_continuous.hip), for the operator-graph voice with or without feedback operators,
// fixed or genes, sots_render_graph.hip (4.16, 4.17, 4.19).  Internal to libsots_hip.so; the public boundary is
// sots_render_overlap_add / sots_render_continuous / sots_render_graph_continuous / sots_render_graph_feedback /
// sots_render_graph_genes in include/sots_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "sots_kernels.h" // SynthParams

namespace sots {

// One pass of the rendering.  The pass holds the audio of chunks first_row .. first_row + rows - 1 in `audio`, a row
// per chunk, `pitch` floats apart; positions are counted from the first sample of chunk first_row ("pass samples":
// chunk l of the pass stands for pass samples [l hop, l hop + n)).  The kernel writes out[j], j < 4 quads, for pass
// samples out_first + j: every chunk of the pass that covers the sample, in ascending order,
//     acc = acc + w[s - l hop] * a_l[s - l hop],  den = den + w[s - l hop],   out = den > 0 ? acc / den : 0
// with w = 1 where window == nullptr.  The caller sees to it that no chunk outside the pass covers a sample it keeps.
// out_first must be a multiple of 4 where hop is (the 16-byte row loads rest on it); out holds 4 quads floats.
struct RenderPass {
    const float *audio;
    const float *window; // N floats, or nullptr: rectangular
    float *out;
    uint32_t rows, hop, n, pitch;
    uint32_t out_first, quads;
};
hipError_t launch_overlap_add(hipStream_t st, const RenderPass &pass);

// Rows a pass may hold whatever the caller asks for: the pass samples stay far below 2^31 and the scratch below 256 MiB.
inline uint32_t render_max_rows(uint32_t pitch)
{
    const uint32_t r = (1u << 26) / pitch;
    return r < 128u ? 128u : r;
}

// Device memory of the renderings, owned by a context: allocated on first use, grown when a call needs more, freed
// with the context.  Apart from these buffers a rendering writes nothing on the device.  The continuous rendering adds
// `words`: its phase buffers, tile totals and carries in one allocation (ContLayout below says where each lies).
struct RenderScratch {
    float *values = nullptr, *audio = nullptr, *out = nullptr;
    size_t values_floats = 0, audio_floats = 0, out_floats = 0;
    uint32_t *words = nullptr;
    size_t words_count = 0;
};
hipError_t render_reserve(RenderScratch &rs, size_t values_floats, size_t audio_floats, size_t out_floats);
hipError_t render_reserve_words(RenderScratch &rs, size_t words);
void render_release(RenderScratch &rs);

// ---- phase-continuous rendering ----
// A pass is `count` consecutive output samples, the first of them sample n0 of the rendering, cut into tiles of
// kContTile samples counted from the pass's first.  Every operator stage of the voice is three launches in stream order:
// reduce (a tile's increments summed to one word), scan (one workgroup per chain: the exclusive prefix of the totals on
// top of the carry the pass before left, and the carry for the pass after), apply (the increments again, scanned inside
// the tile on top of its base: the stage's phase word of every sample, or - the last stage - the output sample).
constexpr uint32_t kContTile = 4096;            // samples per tile = kContThreads lanes x 4 samples
constexpr uint32_t kContMaxPass = 1u << 22;     // samples per pass: 6 phase buffers of 16 MiB at the most (the voice of three chains)
constexpr uint32_t kContMaxChains = 3, kContMaxStages = 4;
constexpr size_t kContMaxValueFloats = 1u << 24; // floats of genes a pass may need on the device (64 MiB)

inline uint32_t cont_chains(uint32_t kind) { return kind == SOTS_SYNTH_TRIPLE_PAR ? 3u : 1u; }

// where the words of a rendering lie in RenderScratch::words, for passes of at most pass_samples samples
struct ContLayout {
    uint32_t stride, tiles; // words between the chains of a phase buffer (a multiple of 4), tiles of a full pass
    size_t phi[2], totals, carry, words;
};
inline ContLayout cont_layout(uint32_t kind, uint32_t pass_samples)
{
    ContLayout l{};
    const uint32_t chains = cont_chains(kind);
    l.stride = (pass_samples + 3u) & ~3u;
    l.tiles = (pass_samples + kContTile - 1u) / kContTile;
    l.phi[0] = 0;
    l.phi[1] = (size_t)chains * l.stride;
    l.totals = 2 * (size_t)chains * l.stride;
    l.carry = l.totals + (((size_t)chains * l.tiles + 3u) & ~(size_t)3u);
    l.words = l.carry + kContMaxStages * kContMaxChains;
    return l;
}

// Row position of sample n (include/sots_hip.h, sots_render_continuous): row k and the r samples behind its anchor
// k hop + N/2; the rendering holds row 0 in front of the first anchor and row num_rows - 1 from the last one on.
__host__ __device__ inline void cont_position(uint32_t n, uint32_t half_n, uint32_t hop, uint32_t num_rows, uint32_t &k, uint32_t &r)
{
    k = 0, r = 0;
    if (n > half_n) {
        const uint32_t m = n - half_n;
        k = m / hop, r = m - k * hop;
        if (k >= num_rows - 1u) k = num_rows - 1u, r = 0;
    }
}

struct ContPass {
    const float *values;    // genes of rows row_base ..., D floats each: every row a sample of the pass looks at
    const float *wavetable; // kWavetableSize floats
    uint32_t *words;        // RenderScratch::words
    float *out;             // count floats (16-byte aligned)
    ContLayout lay;
    uint32_t row_base, num_rows, hop, half_n, glide;
    uint32_t n0, count;
    SynthParams sp;
};
// every stage of one pass; the carries (lay.carry) are the caller's to clear before the first pass
hipError_t launch_continuous_pass(hipStream_t st, uint32_t kind, const ContPass &pass, uint32_t num_cus);

// ---- phase-continuous rendering of the operator-graph voice (sots_render_graph.hip) ----
// Passes, tiles and the three launches are those above, per LEVEL of the graph (graph_levels, sots_rules.h) with the level's
// operators in grid.y; every operator keeps a phase buffer of its own, a word per sample of the pass, and a last launch
// mixes the carriers.  Feedback never touches a phase.  An operator with beta != 0 ("flagged", a bit of fb_mask) has in
// addition a buffer of its shaped values t_j, a float per sample of the pass, that one chain launch per level fills after
// the level's apply and that later levels and the mix read in place of its phase words; and two floats of state, h1 and h2,
// that a pass leaves for the next.  A voice without feedback operators is fb_mask == 0, flagged == 0: no chain launch, and
// neither hist nor a t buffer is ever touched.  Where the words lie, for passes of at most pass_samples samples:
struct GraphLayout {
    uint32_t stride, tiles; // words between the operators' phase buffers (a multiple of 4), tiles of a full pass
    size_t totals, carry;   // phase buffer j lies at j * stride; totals: 8 x tiles; carry: 8 words, by position in GraphLevels::ops
    size_t hist, tbuf, words; // hist: 16 floats behind the carries, h1 h2 per slot; t buffer of the s-th flagged operator (ascending j) at tbuf + s * stride
};
inline GraphLayout graph_layout(uint32_t ops, uint32_t flagged, uint32_t pass_samples)
{
    GraphLayout l{};
    l.stride = (pass_samples + 3u) & ~3u;
    l.tiles = (pass_samples + kContTile - 1u) / kContTile;
    l.totals = (size_t)ops * l.stride;
    l.carry = l.totals + (((size_t)8u * l.tiles + 3u) & ~(size_t)3u);
    l.hist = l.carry + 8u;
    l.tbuf = l.hist + 16u;
    l.words = l.tbuf + (size_t)flagged * l.stride;
    return l;
}
struct GraphPass {
    const float *values;    // genes of rows row_base ..., 2 x operators floats each: every row a sample of the pass looks at
    const float *wavetable; // kWavetableSize floats
    uint32_t *words;        // RenderScratch::words
    float *out;             // count floats (16-byte aligned)
    GraphLayout lay;
    uint32_t row_base, num_rows, hop, half_n, glide;
    uint32_t n0, count;
    SynthParams sp;
    uint32_t fb_mask;   // the flagged operators
    float scaled[8];    // B_j = beta_j K (scale_feedback, sots_rules.h)
    uint32_t forms;     // bit j: operator j's chain runs as a relaxation (else serially)
    uint32_t relax_cap; // sweeps per tile before a tile is finished serially, 1..4096 (read where fb_mask != 0)
};
// A voice whose feedback indices are genes (sots_create_graph_genes): a row of the track is D = 2 x operators
// + E floats.  The pass's rows reach the device in two parts: their first 2 x operators floats in GraphPass::values, which is
// all that reduce, apply and mix look at - they are the kernels of every graph voice, unchanged - and their E gene columns in
// `rows`, E floats per row of the same rows (row_base ...), which only the chains look at.  An operator of `mask` takes B at
// sample n from its column, held or glided and scaled by pass.sp as any gene: effective_feedback(p) K.  Every operator of mask
// is flagged in the pass's fb_mask; the other flagged operators keep pass.scaled.  This stands beside GraphPass and not in it:
// GraphPass is an argument by value of every kernel of the file, and the kernels of a voice without gene operators stay what
// they were, byte for byte.  Only the chain launches of a voice with gene operators take it, kernels of their own.
struct GraphGenes {
    const float *rows;  // the gene columns of the pass's rows, `count` floats each
    uint32_t count;     // E
    uint32_t first;     // 2 x operators: gene column q of a row of D is rows[q - first], and its range pass.sp.pmin/pmax[q]
    uint32_t mask;      // the operators whose index is a gene
    uint32_t column[8]; // by operator: q; read where the operator's bit of mask is set
};
// every level of one pass with its chains, and the mix; the carries (lay.carry) and, where fb_mask != 0, hist are the
// caller's to clear before the first pass.  waveforms: the eight codes (sots_set_voice_waveforms).  genes: null, or with a
// mask of 0, for a voice without gene operators.
hipError_t launch_graph_pass(hipStream_t st, const sots_voice_graph &graph, const uint32_t waveforms[8], const GraphPass &pass, uint32_t num_cus,
                             const GraphGenes *genes = nullptr);

} // namespace sots
