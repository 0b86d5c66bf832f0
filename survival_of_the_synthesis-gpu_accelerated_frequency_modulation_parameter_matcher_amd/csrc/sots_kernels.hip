// sots_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels for the per-generation
// evolutionary FM sound-matching loop.  Compiled with -ffp-contract=off: every fp32
// expression rounds exactly as written, which is what makes synthesis, recombination and
// the value half of mutation bit-identical to the CPU restatement.
//
// Layout choices (DESIGN.md has the reasoning):
//   * variation kernels        : one lane per gene, coalesced [P][D] rows
//   * synthesisePopulation     : one lane per individual (the phase recurrence is serial in
//                                fp32), 128 KiB wavetable staged in LDS, 16-byte row stores
//   * FFT / fitness            : one individual per wavefront, Stockham radix-8/4 passes
//                                (three/two radix-2 layers kept in registers), padded LDS
//                                exchange, xor-shuffle reduction of the squared error
//   * sortPopulation           : bitonic network on (fitness, index) 64-bit keys, LDS tiles
//
// Still the one translation unit of the kernels.  The families are moving into csrc/kernels/*.h, each included where
// its code stood.  Out: common.h, stamps.h, fft.h, objective.h and every family compiled with contraction
// on or standing between two of them - sel_keys.h, spectral_wave.h (k_fft), sort.h, select_tiles.h, select_splitters.h,
// spectral_x.h (k_fft_x), spectral_big.h (k_fft_big).  Such a file states its contraction mode in its first lines and
// ends with contract(off), this unit's default, so no contraction pragma is left in this file.  Still here, all in the
// default mode: variation, synthesis, k_window, the island exchange, and behind the first launchers k_synth_dev,
// k_bucket_fitness and the run record / chunk queue.
//
// Reference citations are file:line in the reference tree.
#include "sots_kernels.h"
#include "sots_stop_rule.h"
#include "kernels/common.h"
#include "kernels/stamps.h"
#include <type_traits>

#include <cstdlib>

namespace sots {

uint32_t next_pow2(uint32_t v)
{
    uint32_t r = 1;
    while (r < v) r <<= 1;
    return r;
}

namespace {

// ------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al. 2011).  Replaces MWC64X (ocl_program.cl:5-16): the state
// is the counter (global individual id, epoch, block, domain) under the key (seed).
// ------------------------------------------------------------------------------------
struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                            uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // one 32 x 32 -> 64-bit multiply per product (v_mad_u64_u32) instead of a high and a low one: integer multiplies
        // run at a quarter of the vector rate and are most of what a gene costs
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        const uint32_t n0 = hi1 ^ c1 ^ k0;
        const uint32_t n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}

__device__ __forceinline__ uint32_t u4_at(const U4 &v, uint32_t i)
{
    return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}

// (float)((int)MWC64X) / 2147483647.0f, ocl_program.cl:27,61
__device__ __forceinline__ float draw_unit(uint32_t w)
{
    return (float)((int32_t)w) / 2147483647.0f;
}

// ------------------------------------------------------------------------------------
// initPopulation, ocl_program.cl:46-66
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_init_population(float *__restrict__ values,
                                                         float *__restrict__ steps,
                                                         float *__restrict__ fitness, PopDims pd,
                                                         uint32_t chunk)
{
    const uint32_t total = pd.p * pd.d;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t i = e / pd.d, g = e - i * pd.d;
        const U4 r = philox4x32_10(pd.gid_base + i, chunk, g >> 2, kTagInit, pd.seed_lo, pd.seed_hi);
        const float u = draw_unit(u4_at(r, g & 3u));
        steps[e] = 0.1f;
        values[e] = (u < 0.0f) ? -u : u;
        if (g == 0) fitness[i] = 0.0f;
    }
}

// ------------------------------------------------------------------------------------
// recombinePopulation, ocl_program.cl:73-149.  Block b copies parent block b % NPB and
// moves gene g of local individual l to local individual (l + g*(b+1)) mod B (:130-137).
// Out of place (current half -> other half): the reference's in-place version lets
// offspring blocks read parent rows that parent blocks are overwriting (:104-147).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t recombine_source(uint32_t i, uint32_t g, const PopDims &pd)
{
    // (g < 16 and b + 1 <= 2^26, so g (b + 1) fits 32 bits; the branches are uniform: pd is a kernel argument)
    uint32_t b, l;
    if (pd.block_shift != kNoPow2) {
        const uint32_t mask = pd.block - 1u;
        b = i >> pd.block_shift;
        l = ((i & mask) - g * (b + 1u)) & mask;
    } else {
        b = i / pd.block;
        const uint32_t dl = i - b * pd.block, shift = (g * (b + 1u)) % pd.block;
        l = (dl + pd.block - shift) % pd.block;
    }
    const uint32_t pb = pd.npb_mask != kNoPow2 ? (b & pd.npb_mask) : b % pd.npb;
    return (pb * pd.block + l) * pd.d + g;
}

// ------------------------------------------------------------------------------------
// mutatePopulation, ocl_program.cl:155-190.  13 draws per gene = Philox blocks 4g..4g+3.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void mutate_gene(float &x, float &s, uint32_t gid, uint32_t g,
                                            uint32_t generation, const PopDims &pd,
                                            const MutateConsts &mc)
{
    const U4 r0 = philox4x32_10(gid, generation, 4u * g + 0u, kTagMutate, pd.seed_lo, pd.seed_hi);
    const U4 r1 = philox4x32_10(gid, generation, 4u * g + 1u, kTagMutate, pd.seed_lo, pd.seed_hi);
    const U4 r2 = philox4x32_10(gid, generation, 4u * g + 2u, kTagMutate, pd.seed_lo, pd.seed_hi);
    const U4 r3 = philox4x32_10(gid, generation, 4u * g + 3u, kTagMutate, pd.seed_lo, pd.seed_hi);
    const bool even = (r0.x % 2u) == 0u;
    const float ek = even ? mc.alpha : mc.one_over_alpha;             // :168
    const float pw = even ? mc.pow_alpha_beta : mc.pow_inv_alpha_beta; // pow(Ek, BETA), :185
    float sum = 0.0f;                                                  // gauss_rand, :21-31
    sum += draw_unit(r0.y); sum += draw_unit(r0.z); sum += draw_unit(r0.w);
    sum += draw_unit(r1.x); sum += draw_unit(r1.y); sum += draw_unit(r1.z); sum += draw_unit(r1.w);
    sum += draw_unit(r2.x); sum += draw_unit(r2.y); sum += draw_unit(r2.z); sum += draw_unit(r2.w);
    sum += draw_unit(r3.x);
    sum /= 12.0f;
    float gauss = sum;
    float new_x = x + ek * s * gauss;                                  // :174
    if (new_x < 0.0f || new_x > 1.0f) {                                // :176-182
        gauss = gauss * -0.5f;
        new_x = x + ek * s * gauss;
    }
    const float es = expf(fabsf(gauss) - mc.root_two_over_pi);         // :184
    s *= pw * powf(es, mc.beta_scale);                                 // :185
    x = new_x;
}

// ------------------------------------------------------------------------------------
// Gene g of individual i of the new half: THE rule of variation, used by every kernel that makes individuals.
// Rows i < pd.survivors (sots_set_survivors; 0 = the reference's strategy) are carried: value and step are bit copies of
// the row's own entry in the sorted current half, nothing is drawn, nothing is mutated.  Every other row is what it is
// without survivors - Philox is counter-based, so the draws the survivors leave out are nobody else's.
// row_base: first element of the individual's population in vin / sin (a batch chunk; 0 in a context).  WHAT: the stage
// kernels do one half each (kVaryMutate alone works in place: the source is the gene's own entry).
// ------------------------------------------------------------------------------------
constexpr uint32_t kVaryRecombine = 1u, kVaryMutate = 2u;
template <uint32_t WHAT = kVaryRecombine | kVaryMutate>
__device__ __forceinline__ void make_gene(float &x, float &s, const float *__restrict__ vin, const float *__restrict__ sin,
                                          uint32_t row_base, uint32_t i, uint32_t g, uint32_t generation, const PopDims &pd,
                                          const MutateConsts &mc)
{
    const bool survivor = i < pd.survivors;
    const uint32_t src = row_base + ((WHAT & kVaryRecombine) && !survivor ? recombine_source(i, g, pd) : i * pd.d + g);
    x = vin[src];
    s = sin[src];
    if ((WHAT & kVaryMutate) && !survivor) mutate_gene(x, s, pd.gid_base + i, g, generation, pd, mc);
}

__global__ __launch_bounds__(256) void k_recombine(const float *__restrict__ vin,
                                                   const float *__restrict__ sin,
                                                   float *__restrict__ vout,
                                                   float *__restrict__ sout, PopDims pd)
{
    const uint32_t total = pd.p * pd.d;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t i = e / pd.d, g = e - i * pd.d;
        float x, s;
        make_gene<kVaryRecombine>(x, s, vin, sin, 0u, i, g, 0u, pd, MutateConsts{});
        vout[e] = x;
        sout[e] = s;
    }
}

__global__ __launch_bounds__(256) void k_mutate(float *__restrict__ values, float *__restrict__ steps,
                                                PopDims pd, MutateConsts mc, uint32_t generation)
{
    const uint32_t total = pd.p * pd.d;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t i = e / pd.d, g = e - i * pd.d;
        float x, s;
        make_gene<kVaryMutate>(x, s, values, steps, 0u, i, g, generation, pd, mc);
        values[e] = x;
        steps[e] = s;
    }
}

__global__ __launch_bounds__(256) void k_recombine_mutate(const float *__restrict__ vin,
                                                          const float *__restrict__ sin,
                                                          float *__restrict__ vout,
                                                          float *__restrict__ sout, PopDims pd,
                                                          MutateConsts mc, uint32_t generation)
{
    const uint32_t total = pd.p * pd.d;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t i = e / pd.d, g = e - i * pd.d;
        float x, s;
        make_gene(x, s, vin, sin, 0u, i, g, generation, pd, mc);
        vout[e] = x;
        sout[e] = s;
    }
}

// ------------------------------------------------------------------------------------
// Chunks in flight (sots_batch): `chunks` populations of pd.p rows each, chunk-major (row r = chunk r / P, local index
// r % P).  Every chunk draws exactly what a context of its own would: initialisation with the chunk's index in the
// counter, variation with the LOCAL index (the mutation counter holds no chunk index, as in the single context).
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_init_population_seg(float *__restrict__ values, float *__restrict__ steps,
                                                             float *__restrict__ fitness, PopDims pd, uint32_t first_chunk,
                                                             uint32_t chunks)
{
    const uint32_t total = chunks * pd.p * pd.d;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t r = e / pd.d, g = e - r * pd.d, c = r / pd.p, i = r - c * pd.p;
        const U4 rn = philox4x32_10(pd.gid_base + i, first_chunk + c, g >> 2, kTagInit, pd.seed_lo, pd.seed_hi);
        const float u = draw_unit(u4_at(rn, g & 3u));
        steps[e] = 0.1f;
        values[e] = (u < 0.0f) ? -u : u;
        if (g == 0) fitness[r] = 0.0f;
    }
}

__global__ __launch_bounds__(256) void k_recombine_mutate_seg(const float *__restrict__ vin, const float *__restrict__ sin,
                                                              float *__restrict__ vout, float *__restrict__ sout, PopDims pd,
                                                              MutateConsts mc, uint32_t generation, uint32_t chunks)
{
    const uint32_t total = chunks * pd.p * pd.d;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t r = e / pd.d, g = e - r * pd.d, c = r / pd.p, i = r - c * pd.p;
        float x, s;
        make_gene(x, s, vin, sin, c * pd.p * pd.d, i, g, generation, pd, mc);
        vout[e] = x;
        sout[e] = s;
    }
}

// Chunk queue (sots_batch_queue_run): slot c runs under a generation counter of its own, slot_table[c] = {chunk index or
// kQueueNoChunk, generations completed}; everything else is k_recombine_mutate_seg.  An idle slot (its chunk retired, the
// queue empty) goes on being varied under its old counter: nothing reads its rows any more.
__global__ __launch_bounds__(256) void k_recombine_mutate_queue(const float *__restrict__ vin, const float *__restrict__ sin,
                                                                float *__restrict__ vout, float *__restrict__ sout, PopDims pd,
                                                                MutateConsts mc, const uint32_t *__restrict__ slot_table, uint32_t slots)
{
    const uint32_t total = slots * pd.p * pd.d;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t r = e / pd.d, g = e - r * pd.d, c = r / pd.p, i = r - c * pd.p;
        float x, s;
        make_gene(x, s, vin, sin, c * pd.p * pd.d, i, g, slot_table[2u * c + 1u], pd, mc);
        vout[e] = x;
        sout[e] = s;
    }
}

// ------------------------------------------------------------------------------------
// synthesisePopulation{,DoubleSeries,TripleParallel}, ocl_program.cl:280-443 /
// Objective::synthesiseAudio*, Evolutionary_Strategy.hpp:368-495.
//
// The oscillator phases are fp32 running sums with a conditional wrap per sample, so a
// voice is serial in the sample index and cannot be split over lanes without changing the
// rounding (and with it table indices and spectra).  The 32768-entry wavetable (128 KiB)
// lives in LDS, one workgroup per CU, which leaves 32 KiB of LDS.  One kernel:
//   k_synth      every voice, one lane per individual.  A voice is J parallel chains of OPS
//                operators in series; operator s of block k-s runs in loop trip k (software
//                pipeline over blocks of 8 samples, two alternating register sets, no copies),
//                so no table read is waited for in the trip that issues it.  Finished samples
//                are parked in a swizzled LDS tile and leave as whole 128-byte lines.
//                For small populations a series chain is cut into two wavefronts (SPLIT, below).
// With one wavefront per SIMD every vector instruction costs four cycles, whatever it does, so
// the instruction count per sample is what the loop time follows (in-kernel s_memtime stamps,
// -DSOTS_STAMP): branch-free wraps (below), packed v_pk_* arithmetic for the per-sample
// mul/add/mul outside the recurrences.  Every per-sample operation is the reference's, in
// its order, unfused, so the audio is bit-identical to the serial loop.
// ------------------------------------------------------------------------------------
#ifndef SOTS_SYNTH_UNROLL
#define SOTS_SYNTH_UNROLL 8
#endif
constexpr int kSynthUnroll = SOTS_SYNTH_UNROLL; // samples per pipeline block
#ifndef SOTS_SYNTH_UNROLL_CUT
#define SOTS_SYNTH_UNROLL_CUT 16
#endif
// ... and of a chain cut over several wavefronts: a trip there ends in a workgroup barrier and starts with the read of
// the block handed over (together about 400 cycles), so longer blocks halve the number of trips
constexpr int kSynthUnrollCut = SOTS_SYNTH_UNROLL_CUT;
constexpr float kWf = (float)kWavetableSize;

// table[clamp((int)pos, 0, W-1)]; CLAMP = false only where the phase is known to be in [0, W)
template <bool CLAMP = true>
__device__ __forceinline__ float tab_at(const float *tab, float pos)
{
    if constexpr (CLAMP) {
        // (round 4: v_cvt_u32_f32 + v_min_u32 - a saturating conversion and a two-operand minimum, as k_synth_ol does it - measures
        // SLOWER here: 52.2 against 51.3 us at P = 65 536, 99 against 95 at 131 072; the asm statement costs the scheduler more than
        // the cheaper minimum brings)
        int i = (int)pos; // == (unsigned)pos for every in-range phase
        i = min(max(i, 0), (int)kWavetableSize - 1);
        return tab[i];
    } else {
        return tab[(uint32_t)pos];
    }
}
// The reference's two conditional wraps, `if (p >= W) p -= W;` and `if (p < 0) p += W;`, as
// subtract/add and an UNSIGNED INTEGER minimum of the bit patterns.  Non-negative floats order
// like their bit patterns and every negative float is a larger unsigned number than every
// non-negative one.  The subtraction and addition are the reference's own fp32 operations, so
// the result carries its rounding.
//   wrap_hi (first wrap only, 2 instructions instead of 3): p >= W -> 0 <= p-W < p picks p-W;
//     0 <= p < W -> p-W < 0 picks p;  p < 0 -> p-W is further from zero than p, picks p.
//   wrap_both (both wraps, 3 instructions instead of 6, and the phase recurrence becomes
//     add -> {sub, add} -> v_min3_u32):  p >= W -> the reference takes p-W, which is >= 0 so its
//     second wrap does nothing, and p-W is the smallest pattern;  0 <= p < W -> it keeps p, p-W
//     is negative and p+W larger;  p < 0 -> it takes p+W, which is non-negative or closer to
//     zero than p and p-W.
// The one bit pattern that would differ is p == -0.0f in wrap_both (the reference keeps it, this
// gives W): a phase starts at +0.0f and x + y is -0.0f only when both are, so it never occurs.
__device__ __forceinline__ void wrap_hi(float &p)
{
    p = __uint_as_float(min(__float_as_uint(p - kWf), __float_as_uint(p)));
}
__device__ __forceinline__ void wrap_both(float &p)
{
    const v2f_t bc = v2f_t{p, p} + v2f_t{-kWf, kWf}; // one v_pk_add_f32
    p = __uint_as_float(min(min(__float_as_uint(bc.x), __float_as_uint(bc.y)), __float_as_uint(p)));
}

// ---- every voice, one lane per individual, whole-line stores through LDS -------------------
// Each wavefront owns an 8 KiB tile [64 rows][8 chunks of 16 B], XOR-swizzled by row so that
// both the row-wise writes (lane = row) and the transposed reads (lane = 8 rows x 8 chunks) are
// bank-conflict free.  Every 32 samples the tile is read back transposed and written with
// stores in which 8 neighbouring lanes cover one whole 128-byte line of one row.  (The
// row-per-lane 16-byte store it replaces touches 64 lines per instruction and 8 L2 requests
// per line: 91 us instead of 57 us for the 2-operator voice at P = 65536.)
constexpr int kSynthWaves = 4;  // at most: one per SIMD, 4 x 8 KiB of tiles beside the table
constexpr int kStageChunks = 8; // 16-byte chunks per row per flush = 32 samples

template <int KIND> struct VoiceShape;
template <> struct VoiceShape<SOTS_SYNTH_2OP> { static constexpr int J = 1, OPS = 2, D = 4; };
template <> struct VoiceShape<SOTS_SYNTH_3OP_SERIES> { static constexpr int J = 1, OPS = 3, D = 6; };
template <> struct VoiceShape<SOTS_SYNTH_4OP_SERIES> { static constexpr int J = 1, OPS = 4, D = 8; };
template <> struct VoiceShape<SOTS_SYNTH_TRIPLE_PAR> { static constexpr int J = 3, OPS = 2, D = 12; };


// SPLIT > 0 (series voices, at most two wavefronts' worth of individuals per CU): the chain is cut in
// front of operator SPLIT and runs in TWO wavefronts per 64 individuals, so that all four SIMDs of
// a CU work when the population is small.  The FRONT wavefront runs operators 0..SPLIT-1 and hands
// c * (t * mul + off) - operator SPLIT's phase increments, the same unfused arithmetic - over
// through LDS, one 8-sample block per trip; the BACK wavefront runs operators SPLIT..OPS-1 and
// the tile.  Both execute the same sequence of trips with one workgroup barrier per trip: the
// block handed over in trip k is consumed in trip k+1, exactly when the one-wavefront pipeline
// would read it from registers, and the two hand-over buffers alternate with the block parity.
// HELP (fused generation loop, 4-gene voice, one or two tiles per workgroup): the workgroup starts with four times its
// wavefronts (sixteen for a full tile); each thread makes one gene of the tile's individuals (recombination source, 13 Philox draws, exp, pow), so
// the variation runs once across 1024 lanes at four wavefronts per SIMD instead of four times in a row in each of
// 256 lanes at one; the twelve extra wavefronts then leave and the usual four synthesise.
// SPLIT2 > SPLIT: a second cut in front of operator SPLIT2 - three wavefronts per 64 individuals (stages of operators
// [0, SPLIT), [SPLIT, SPLIT2), [SPLIT2, OPS)), two hand-over links; for the 4-operator voice at <= 128 individuals per CU
// where a series chain of OPS operators is cut, as compile-time facts
// SPLIT3 > SPLIT2: a third cut - with SPLIT = 1, 2, 3 every operator of the 4-operator voice has a wavefront of its own,
// four wavefronts per 64 individuals and three links: eight wavefronts for the 128 individuals per CU of BASELINE configs[3]'s
// shard, two per SIMD (one wavefront alone on a SIMD issues an instruction every ~4.5 cycles, two sharing it every ~2.3).
// The 32 KiB beside the table then hold 2 tiles of 4 KiB (16 samples, leaving as half lines) and 6 hand-over buffers of
// 4 KiB (two 8-sample blocks each).
template <int SPLIT, int SPLIT2, int SPLIT3, int OPS> struct CutPlan {
    static constexpr int STAGES = 1 + (SPLIT > 0 ? 1 : 0) + (SPLIT2 > 0 ? 1 : 0) + (SPLIT3 > 0 ? 1 : 0);
    static constexpr int cuts_before(int S) { return (SPLIT > 0 && S >= SPLIT ? 1 : 0) + (SPLIT2 > 0 && S >= SPLIT2 ? 1 : 0) + (SPLIT3 > 0 && S >= SPLIT3 ? 1 : 0); }
    // stage of operator S: 0 = the chain's head ... STAGES-1 = its tail (which also owns the tile)
    static constexpr int stage_of(int S) { return cuts_before(S); }
    // In trip k operator S works on block k - slot(S): one trip behind the operator in front of it, TWO behind it
    // across a cut (the stage in front sends a block in the trip AFTER it read the table for it, when the values
    // have landed, and the block is read in the trip after that); block k - slot(OPS) leaves.
    static constexpr int slot(int S) { return S + cuts_before(S); }
    static constexpr bool is_cut(int S) { return S > 0 && (S == SPLIT || S == SPLIT2 || S == SPLIT3); }
    static constexpr bool consumes(int S) { return SPLIT > 0 && is_cut(S); }
    static constexpr bool produces(int S) { return SPLIT > 0 && S + 1 < OPS && is_cut(S + 1); }
    // samples per pipeline block and 16-byte chunks per tile row: the deepest cut has the least LDS per buffer
    static constexpr int U = SPLIT == 0 ? kSynthUnroll : STAGES >= 4 ? 8 : kSynthUnrollCut;
    static constexpr int CH = STAGES >= 4 ? 4 : kStageChunks;
};

template <int KIND, int SPLIT, bool HELP = false, int SPLIT2 = 0, int SPLIT3 = 0>
__global__ __launch_bounds__((HELP ? (SPLIT ? 8 : 16) : SPLIT3 ? 8 : SPLIT2 ? 6 : 4) * kWave) void k_synth(const float *__restrict__ values,
                                                               const float *__restrict__ wavetable,
                                                               float *__restrict__ audio, SynthParams sp,
                                                               uint32_t p_len, uint32_t n, uint32_t pitch, Variation var)
{
    constexpr int J = VoiceShape<KIND>::J, OPS = VoiceShape<KIND>::OPS, D = VoiceShape<KIND>::D;
    // SPLIT < 0 (the voice of J parallel chains, up to 64 individuals per CU): a wavefront per CHAIN.  Every wavefront runs
    // its chain's operators as the uncut pipeline does; the chains of wavefronts 1 ... J-1 hand gain * (table value) - the
    // reference's product - to wavefront 0 through LDS, one block per trip and one workgroup barrier per trip as in the
    // series cuts, and wavefront 0 adds them to its own in the reference's order and owns the tile.
    constexpr bool PSPLIT = SPLIT < 0;
    using Plan = CutPlan<(PSPLIT ? 0 : SPLIT), SPLIT2, SPLIT3, OPS>;
    constexpr int U = PSPLIT ? kSynthUnrollCut : Plan::U;
    constexpr int CH = PSPLIT ? kStageChunks : Plan::CH; // 16-byte chunks per tile row = 4 CH samples per flush
    constexpr int RPI = kWave / CH;     // rows per transposed read / store instruction (CH of them per flush)
    static_assert(U % 4 == 0 && 4 * CH % U == 0, "whole 16-byte chunks, whole blocks per flush");
    static_assert(SPLIT <= 0 || (J == 1 && SPLIT < OPS), "only a series chain can be cut");
    static_assert(!PSPLIT || (J == 3 && OPS == 2 && !HELP && SPLIT2 == 0), "the parallel split serves the three 2-operator chains");
    static_assert(SPLIT2 == 0 || (SPLIT > 0 && SPLIT2 > SPLIT && SPLIT2 < OPS), "the second cut lies behind the first");
    static_assert(SPLIT3 == 0 || (SPLIT2 > 0 && SPLIT3 > SPLIT2 && SPLIT3 < OPS), "the third cut lies behind the second");
    static_assert(!HELP || SPLIT > 0 || D == 4, "uncut, the helper wavefronts serve the 4-gene voice (128 registers with 16 wavefronts)");
    constexpr uint32_t HT = 4; // HELP: threads per individual while the genes are made (each takes genes t % 4, t % 4 + 4, ...)
    constexpr int STAGES = PSPLIT ? J : Plan::STAGES; // wavefronts per 64 individuals
    __shared__ float tab[kWavetableSize];
    __shared__ float4 stage_all[kSynthWaves * kWave * kStageChunks];
    SOTS_PHASE_BEGIN();
    SOTS_PHASE_REAL(10);
    request_wavetable(tab, wavetable);
    bool table_pending = true; // the first tile's parameters are fetched while the table is on its way
    const float c = (float)kWavetableSize / (float)SOTS_SAMPLE_RATE; // w2srRatio, Evolutionary_Strategy.hpp:203
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave_id = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    // cut kernels: wavefronts [0, pairs) are the TAIL stage, [pairs, 2 pairs) the stage before it, ... of the same 64 individuals
    const uint32_t pairs = HELP ? blockDim.x / (HT * kWave) : blockDim.x / (STAGES * kWave);
    // HELP: the tiles this workgroup will synthesise (1 or 2: blockIdx, blockIdx + gridDim)
    const uint32_t help_tiles = HELP ? (blockIdx.x * (pairs * kWave) + gridDim.x * (pairs * kWave) < p_len ? 2u : 1u) : 0u;
    if constexpr (HELP) {
        // one gene per thread and tile; values and steps go to the other half, the values also to LDS for the
        // wavefronts that stay (the tile area is free until the first samples are parked; they take the second tile's
        // values into registers before they start on the first)
        float *__restrict__ made = reinterpret_cast<float *>(stage_all);
        const uint32_t t = threadIdx.x, li = t / HT; // the individual inside the tile
        for (uint32_t kt = 0; kt < help_tiles; ++kt) {
            const uint32_t i1 = (blockIdx.x + kt * gridDim.x) * (pairs * kWave) + li;
            if (i1 < p_len) {
                for (uint32_t g1 = t % HT; g1 < (uint32_t)D; g1 += HT) {
                    float x, st;
                    make_gene(x, st, var.vin, var.sin, 0u, i1, g1, var.generation, var.pd, var.mc);
                    var.vout[(size_t)i1 * D + g1] = x;
                    var.sout[(size_t)i1 * D + g1] = st;
                    made[kt * (pairs * kWave * D) + li * D + g1] = x;
                }
            }
        }
        __syncthreads();
        SOTS_PHASE(12); // the individuals are made
        if (wave_id >= STAGES * pairs) { // (a cut kernel keeps a wavefront per stage)
            __builtin_amdgcn_s_waitcnt(0); // this wavefront's pieces of the table have landed before it leaves
            return;
        }
    }
    const uint32_t rho = SPLIT ? wave_id / pairs : 0u;          // 0: tail stage
    const int my_stage = STAGES - 1 - (int)rho; // (pairing the tail with the head stage on a SIMD instead: no difference, profiles/r03_experiments.md)
    const bool front = my_stage != STAGES - 1;                  // not the tail: no tile, no stores
    const uint32_t wave = wave_id - rho * pairs;                // which 64 individuals of the workgroup's tile
    float4 *__restrict__ stage = stage_all + wave * kWave * CH;
    // hand-over buffers [link][pair][parity][U/4][lane] of 16 bytes behind the tiles of a cut kernel (launch_synth keeps
    // pairs * (tile + links * hand-over buffer) inside stage_all: two pairs with one link, one pair with two, two pairs
    // with three links of half-length blocks and half-length tiles)
    float4 *__restrict__ xbuf0 = stage_all + pairs * kWave * CH + wave * (2 * (U / 4) * kWave);
    float4 *__restrict__ xbuf1 = xbuf0 + pairs * (2 * (U / 4) * kWave);
    float4 *__restrict__ xbuf2 = xbuf1 + pairs * (2 * (U / 4) * kWave);
    // write side: lane = row; chunk q of the row lives in slot q ^ swz(row): row & 7 with eight chunks, (row >> 1) & 3 with four
    auto swz = [](uint32_t row) { return CH == 8 ? (row & 7u) : ((row >> 1) & 3u); };
    float4 *__restrict__ wr = stage + lane * CH;
    const uint32_t l7 = swz(lane);
    // read side: lane = (row within a group of RPI rows, chunk): group `it` adds 64 slots
    const uint32_t r8 = lane / CH, rch = lane % CH;
    const float4 *__restrict__ rd = stage + r8 * CH + (rch ^ swz(r8)); // (RPI is a multiple of what swz looks at: the group index drops out)
    const uint32_t lane_off = r8 * pitch + 4u * rch; // floats, relative to the group's first row
    uint32_t row_off[CH];                           // ... and, in BYTES, of this lane's piece of a line in each of the CH groups of RPI rows
#pragma unroll
    for (uint32_t g = 0; g < (uint32_t)CH; ++g) row_off[g] = (lane_off + g * RPI * pitch) * 4u; // < 2^32: 64 rows of at most 8224 floats

    const uint32_t rows_per_block = pairs * kWave;
    float help_next[HELP ? D : 1]; // HELP: the second tile's values
    for (uint32_t base = blockIdx.x * rows_per_block; base < p_len; base += gridDim.x * rows_per_block) {
        const uint32_t row0 = base + wave * kWave; // first row of this wavefront
        const uint32_t ind = row0 + lane < p_len ? row0 + lane : p_len - 1u;
        const bool full = row0 + kWave <= p_len; // every row of the tile exists
        float p[D];
        if constexpr (HELP) {
            if (base == blockIdx.x * rows_per_block) { // first tile: both tiles' values leave LDS now
                const float *__restrict__ made = reinterpret_cast<const float *>(stage_all);
#pragma unroll
                for (int g = 0; g < D; ++g) {
                    p[g] = made[(wave * kWave + lane) * D + g];
                    help_next[g] = help_tiles > 1 ? made[rows_per_block * D + (wave * kWave + lane) * D + g] : 0.0f;
                }
            } else {
#pragma unroll
                for (int g = 0; g < D; ++g) p[g] = help_next[g];
            }
        } else if (var.vin) {
            // fused generation loop: this lane's individual is made here (k_recombine_mutate's
            // arithmetic, gene by gene) and written to the other half by the wavefront that owns the row
            const bool owner = !front && row0 + lane < p_len;
#pragma unroll 1
            for (int g = 0; g < D; ++g) {
                float x, st;
                make_gene(x, st, var.vin, var.sin, 0u, ind, (uint32_t)g, var.generation, var.pd, var.mc);
                if (owner) {
                    var.vout[(size_t)ind * D + g] = x;
                    var.sout[(size_t)ind * D + g] = st;
                }
                p[g] = x;
            }
        } else {
#pragma unroll
            for (int g = 0; g < D; ++g) p[g] = values[(size_t)ind * D + g];
        }
#pragma unroll
        for (int g = 0; g < D; ++g) {
            // scaleParams: min + v*(max-min), ocl_program.cl:297; the triple voice scales all
            // three 2-op voices by entries 0..3, Evolutionary_Strategy.hpp:453-455
            const int sc = KIND == SOTS_SYNTH_TRIPLE_PAR ? (g & 3) : g;
            p[g] = sp.pmin[sc] + p[g] * (sp.pmax[sc] - sp.pmin[sc]);
        }
        // Operator 0 of chain j runs free at inc0[j]; operator s >= 1 advances by
        // c * (t_prev * mul[s][j] + off[s][j]); the output is gain[j] * (last operator's table value).
        float inc0[J], mul[OPS][J], off[OPS][J], gain[J];
        if constexpr (KIND == SOTS_SYNTH_2OP) { // Evolutionary_Strategy.hpp:372-401
            inc0[0] = c * p[0], mul[1][0] = p[0] * p[1], off[1][0] = p[2], gain[0] = p[3];
        } else if constexpr (KIND == SOTS_SYNTH_TRIPLE_PAR) { // :457-494
#pragma unroll
            for (int j = 0; j < J; ++j)
                inc0[j] = c * p[4 * j], mul[1][j] = p[4 * j] * p[4 * j + 1], off[1][j] = p[4 * j + 2], gain[j] = p[4 * j + 3];
        } else { // series, :407-445 (the 4-operator voice adds one more modulator stage)
            inc0[0] = c * p[1];
#pragma unroll
            for (int o = 1; o < OPS; ++o) mul[o][0] = p[2 * (o - 1)] * p[2 * (o - 1) + 1], off[o][0] = p[2 * (o - 1) + 3];
            gain[0] = p[2 * (OPS - 1)] * p[2 * (OPS - 1) + 1];
        }
        // a free-running phase stays inside [0, W) when 0 <= inc0 < W: its index needs no clamp
        // (round 4: the modulated phases likewise, where every increment they can receive is bounded by c (|mul| + |off|) < W - the
        // unsigned conversion and one two-operand minimum instead of the signed one and v_med3_i32: no difference here, 51.0-51.3
        // against 51.3-51.4 us; k_synth_ol, where the index goes clamp-FREE on that condition, gains 8 %)
        bool in_range = true;
#pragma unroll
        for (int j = 0; j < J; ++j) in_range = in_range && inc0[j] >= 0.0f && inc0[j] < kWf;
        const bool free_unclamped = __all(in_range);
        if (table_pending) {
            wavetable_ready();
            table_pending = false;
            SOTS_PHASE(13); // the table is in LDS
        }
        SOTS_STAMP_SCOPE(blockIdx.x * (blockDim.x / kWave) + wave_id);

        auto run = [&](auto unclamped_tag, auto stage_tag) {
            constexpr bool UNCLAMPED = decltype(unclamped_tag)::value;
            constexpr int MY = decltype(stage_tag)::value; // this wavefront's stage, a compile-time fact in here: its loop holds
                                                          // (and keeps registers for) its own operators only
            constexpr int CHAIN = PSPLIT ? STAGES - 1 - MY : 0; // parallel split: this wavefront's chain (the tail runs chain 0)
            float pos[OPS][J];
#pragma unroll
            for (int o = 0; o < OPS; ++o)
#pragma unroll
                for (int j = 0; j < J; ++j) pos[o][j] = 0.0f;
            float T[OPS][2][J][U]; // table values of operator s, block parity, chain, sample
            v2f_t handed[U / 2];   // cut kernels: the increments fetched for this wavefront's first operator
            v2f_t to_hand[U / 2];  // ... and the ones made for the next stage's
            v2f_t handed2[PSPLIT ? U / 2 : 1]; // parallel split: handed = chain 1's products, handed2 = chain 2's
            // parallel split: this chain's products of its block of parity B (table values read one trip ago) ...
            auto par_make = [&](auto b_tag) {
                constexpr int B = decltype(b_tag)::value;
                if constexpr (PSPLIT && CHAIN != 0) {
#pragma unroll
                    for (int u = 0; u < U; u += 2)
                        to_hand[u / 2] = v2f_t{T[OPS - 1][B][CHAIN][u], T[OPS - 1][B][CHAIN][u + 1]} * gain[CHAIN];
                }
            };
            // ... go to the tail through this chain's link (chain 1: xbuf0, chain 2: xbuf1) ...
            auto par_send = [&](auto b_tag) {
                constexpr int B = decltype(b_tag)::value;
                if constexpr (PSPLIT && CHAIN != 0) {
                    float4 *__restrict__ xout = CHAIN == 1 ? xbuf0 : xbuf1;
#pragma unroll
                    for (int u = 0; u < U; u += 4)
                        xout[(B * (U / 4) + u / 4) * kWave + lane] =
                            make_float4(to_hand[u / 2].x, to_hand[u / 2].y, to_hand[u / 2 + 1].x, to_hand[u / 2 + 1].y);
                }
            };
            // ... where the tail picks both up one trip later
            auto par_fetch = [&](auto b_tag) {
                constexpr int B = decltype(b_tag)::value;
                if constexpr (PSPLIT && CHAIN == 0) {
#pragma unroll
                    for (int u = 0; u < U; u += 4) {
                        const float4 q1 = xbuf0[(B * (U / 4) + u / 4) * kWave + lane], q2 = xbuf1[(B * (U / 4) + u / 4) * kWave + lane];
                        handed[u / 2] = v2f_t{q1.x, q1.y}, handed[u / 2 + 1] = v2f_t{q1.z, q1.w};
                        handed2[u / 2] = v2f_t{q2.x, q2.y}, handed2[u / 2 + 1] = v2f_t{q2.z, q2.w};
                    }
                }
            };

            // Schedule (CutPlan): operator S works on block k - slot(S) in trip k.  A block's parity (which half of T,
            // which hand-over buffer) is its index & 1.
            // link = the producer's stage: stage 0 sends through xbuf0, stage 1 through xbuf1, stage 2 through xbuf2
            auto link_of = [&](int producer) -> float4 * { return Plan::stage_of(producer) == 0 ? xbuf0 : Plan::stage_of(producer) == 1 ? xbuf1 : xbuf2; };

            // the increments of operator S's block (parity B), asked for at the start of the trip
            auto fetch = [&](auto s_tag, auto b_tag) {
                constexpr int S = decltype(s_tag)::value, B = decltype(b_tag)::value;
                if constexpr (Plan::consumes(S) && Plan::stage_of(S) == MY) {
                    const float4 *__restrict__ xin = link_of(S - 1);
#pragma unroll
                    for (int u = 0; u < U; u += 4) {
                        const float4 q = xin[(B * (U / 4) + u / 4) * kWave + lane];
                        handed[u / 2] = v2f_t{q.x, q.y}, handed[u / 2 + 1] = v2f_t{q.z, q.w};
                    }
                }
            };
            // operator S + 1's increments from operator S's block of parity B (read from the table one trip ago):
            // c * (t * mul + off), the reference's mul, add, mul, unfused, two samples per packed instruction
            auto make_handover = [&](auto s_tag, auto b_tag) {
                constexpr int S = decltype(s_tag)::value, B = decltype(b_tag)::value;
                if constexpr (Plan::produces(S) && Plan::stage_of(S) == MY) {
                    constexpr int NX = S + 1 < OPS ? S + 1 : S;
#pragma unroll
                    for (int u = 0; u < U; u += 2)
                        to_hand[u / 2] = (v2f_t{T[S][B][0][u], T[S][B][0][u + 1]} * mul[NX][0] + off[NX][0]) * c;
                }
            };
            auto send_handover = [&](auto s_tag, auto b_tag) {
                constexpr int S = decltype(s_tag)::value, B = decltype(b_tag)::value;
                if constexpr (Plan::produces(S) && Plan::stage_of(S) == MY) {
                    float4 *__restrict__ xout = link_of(S);
#pragma unroll
                    for (int u = 0; u < U; u += 4)
                        xout[(B * (U / 4) + u / 4) * kWave + lane] =
                            make_float4(to_hand[u / 2].x, to_hand[u / 2].y, to_hand[u / 2 + 1].x, to_hand[u / 2 + 1].y);
                }
            };
            // operator S on its block of parity B
            auto op = [&](auto s_tag, auto b_tag) {
                constexpr int S = decltype(s_tag)::value, B = decltype(b_tag)::value;
                if constexpr (PSPLIT || Plan::stage_of(S) == MY) // else: another wavefront's operator
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    if (PSPLIT && j != CHAIN) continue; // (compile-time after unrolling: another wavefront's chain)
                    if constexpr (S == 0) {
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            T[0][B][j][u] = tab_at<!UNCLAMPED>(tab, pos[0][j]);
                            pos[0][j] += inc0[j];
                            wrap_hi(pos[0][j]);
                        }
                    } else {
                        // phase increments, two samples per packed instruction (v_pk_mul_f32,
                        // v_pk_add_f32, v_pk_mul_f32: the reference's mul, add, mul, unfused)
                        v2f_t inc[U / 2];
                        if constexpr (Plan::consumes(S)) { // handed over by the wavefront of the stage in front
#pragma unroll
                            for (int u = 0; u < U; u += 2) inc[u / 2] = handed[u / 2];
                        } else {
#pragma unroll
                            for (int u = 0; u < U; u += 2)
                                inc[u / 2] = (v2f_t{T[S - 1][B][j][u], T[S - 1][B][j][u + 1]} * mul[S][j] + off[S][j]) * c;
                        }
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            T[S][B][j][u] = tab_at(tab, pos[S][j]);
                            pos[S][j] += (u & 1) ? inc[u / 2].y : inc[u / 2].x;
                            wrap_both(pos[S][j]);
                        }
                    }
                }
            };
            // a tile on its way out: eight rows x 128-byte lines per store instruction, the address a wavefront-uniform
            // line start plus a per-lane offset that never changes (no vector address arithmetic per flush)
            float pend[CH][4]; // (plain floats: an array of float4 does not leave memory for registers)
            float *__restrict__ pend_line = audio;
            bool pending = false;
            auto store_pending = [&]() {
                if constexpr (MY != STAGES - 1) return;
                if (!pending) return;
                pending = false;
#pragma unroll
                for (int g = 0; g < CH; ++g) {
                    asm volatile("" : "+v"(row_off[g])); // the zero-extension stays next to the store: scalar base + 32-bit lane offset
                    *reinterpret_cast<float4 *>(reinterpret_cast<char *>(pend_line) + row_off[g]) = make_float4(pend[g][0], pend[g][1], pend[g][2], pend[g][3]);
                }
            };
            // samples ip..ip+U-1 (the block of parity B) leave
            auto emit = [&](auto b_tag, uint32_t ip) {
                constexpr int B = decltype(b_tag)::value;
                if constexpr (MY != STAGES - 1) return; // only the tail stage has samples
                float y[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if constexpr (PSPLIT) // chains 1 and 2 arrive as products from their wavefronts: the same sum in the same order
                        y[u] = (T[OPS - 1][B][0][u] * gain[0] + ((u & 1) ? handed[u / 2].y : handed[u / 2].x) +
                                ((u & 1) ? handed2[u / 2].y : handed2[u / 2].x)) / 3.0f;
                    else if constexpr (KIND == SOTS_SYNTH_TRIPLE_PAR)
                        y[u] = (T[OPS - 1][B][0][u] * gain[0] + T[OPS - 1][B][1][u] * gain[1] + T[OPS - 1][B][2][u] * gain[2]) /
                               3.0f; // == (float)(double(sum)/3.0), :493
                    else
                        y[u] = T[OPS - 1][B][0][u] * gain[0];
                }
                store_pending(); // the tile read back one trip ago leaves now: its LDS reads have long landed
                const uint32_t c0 = (ip >> 2) & (CH - 1);
#pragma unroll
                for (int q = 0; q < U / 4; ++q) wr[(c0 + q) ^ l7] = make_float4(y[4 * q], y[4 * q + 1], y[4 * q + 2], y[4 * q + 3]);
                if (c0 == CH - U / 4) { // 4 CH samples parked: flush the tile
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("" ::: "memory");
                    const uint32_t i0 = ip + U - 4 * CH;
                    float *__restrict__ line0 = audio + (size_t)row0 * pitch + i0; // wavefront-uniform
                    if (full) {
                        // read back transposed now (LDS works in order: the next samples are parked behind these
                        // reads), stored in the next trip
                        constexpr int G = RPI * CH; // slots per group of RPI rows (= 64)
#pragma unroll
                        for (int g = 0; g < CH; ++g) {
                            const float4 q = rd[g * G];
                            pend[g][0] = q.x, pend[g][1] = q.y, pend[g][2] = q.z, pend[g][3] = q.w;
                        }
                        pend_line = line0;
                        pending = true;
                    } else { // last, partly filled tile of the population
#pragma unroll 1
                        for (uint32_t it = 0; it < (uint32_t)CH; ++it)
                            if (row0 + RPI * it + r8 < p_len)
                                *reinterpret_cast<float4 *>(line0 + lane_off + (size_t)(RPI * it) * pitch) = rd[it * RPI * CH];
                    }
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("" ::: "memory");
                }
            };
            const uint32_t nb = n / U; // even and >= 32
            // the slot in which a block leaves; parallel split: one trip later than the uncut pipeline (the other chains' products
            // are made in slot OPS and read in slot OPS + 1; the tail's own table values of that block live until the operator
            // of the same parity overwrites them later in the same trip: the samples leave first)
            constexpr int LAST = PSPLIT ? OPS + 1 : Plan::slot(OPS);
            // Trip k of parity Q.  EDGE (the first and last trips): a slot only works while its block index lies in
            // [0, nb).  Cut kernels: what a wavefront waits for from another stage is asked for first, work that does
            // not need it comes next (the hand-over arithmetic of the block read one trip ago, the samples that leave),
            // then the operators; the hand-over is written last, and only a wavefront that wrote one waits for its LDS
            // operations before the barrier (the tail stage keeps its table reads in flight across it).
            auto trip = [&](auto q_tag, auto edge_tag, uint32_t k) {
                constexpr int Q = decltype(q_tag)::value;
                constexpr bool EDGE = decltype(edge_tag)::value;
                auto on = [&](int sl) { return !EDGE || (k >= (uint32_t)sl && k - (uint32_t)sl < nb); };
                auto each_op = [&](auto &&f, auto shift_tag) { // f(S, parity of the block of slot(S) + shift) where that block exists
                    constexpr int SH = decltype(shift_tag)::value;
                    if (on(Plan::slot(0) + SH)) f(ic<0>{}, ic<(Q ^ ((Plan::slot(0) + SH) & 1))>{});
                    if constexpr (OPS > 1) if (on(Plan::slot(1) + SH)) f(ic<1>{}, ic<(Q ^ ((Plan::slot(1) + SH) & 1))>{});
                    if constexpr (OPS > 2) if (on(Plan::slot(2) + SH)) f(ic<2>{}, ic<(Q ^ ((Plan::slot(2) + SH) & 1))>{});
                    if constexpr (OPS > 3) if (on(Plan::slot(3) + SH)) f(ic<3>{}, ic<(Q ^ ((Plan::slot(3) + SH) & 1))>{});
                };
                if constexpr (PSPLIT) {
                    if (on(LAST)) par_fetch(ic<(Q ^ (LAST & 1))>{});
                    if (on(OPS)) par_make(ic<(Q ^ (OPS & 1))>{});
                    if (on(LAST)) emit(ic<(Q ^ (LAST & 1))>{}, (k - LAST) * U);
                    each_op(op, ic<0>{});
                    if (on(OPS)) par_send(ic<(Q ^ (OPS & 1))>{});
                    asm volatile("" ::: "memory");
                    if constexpr (CHAIN != 0) __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0): the products are in LDS
                    __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
                } else if constexpr (SPLIT > 0) {
                    each_op(fetch, ic<0>{});
                    each_op(make_handover, ic<1>{}); // the block this operator read the table for one trip ago
                    if (on(LAST)) emit(ic<(Q ^ (LAST & 1))>{}, (k - LAST) * U);
                    each_op(op, ic<0>{});
                    each_op(send_handover, ic<1>{});
                    asm volatile("" ::: "memory");
                    if constexpr (MY != STAGES - 1) __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0): the hand-over is in LDS
                    __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
                } else {
                    each_op(op, ic<0>{});
                    if (on(LAST)) emit(ic<(Q ^ (LAST & 1))>{}, (k - LAST) * U);
                }
            };
            constexpr uint32_t K0 = (LAST + 1) & ~1; // first trip with every slot busy, rounded to even
            for (uint32_t k = 0; k < K0; k += 2) {
                trip(ic<0>{}, std::true_type{}, k);
                trip(ic<1>{}, std::true_type{}, k + 1);
            }
            for (uint32_t k = K0; k < nb; k += 2) {
                trip(ic<0>{}, std::false_type{}, k);
                trip(ic<1>{}, std::false_type{}, k + 1);
            }
            for (uint32_t k = nb; k < nb + K0; k += 2) { // the last block leaves in trip nb - 1 + LAST
                trip(ic<0>{}, std::true_type{}, k);
                trip(ic<1>{}, std::true_type{}, k + 1);
            }
            store_pending();
        };
        auto run_my_stage = [&](auto unclamped_tag) {
            if constexpr (STAGES == 1) run(unclamped_tag, ic<0>{});
            else if (my_stage == 0) run(unclamped_tag, ic<0>{});
            else if (STAGES == 2 || my_stage == 1) run(unclamped_tag, ic<1>{});
            else if (STAGES == 3 || my_stage == 2) run(unclamped_tag, ic<(STAGES > 2 ? 2 : 0)>{});
            else run(unclamped_tag, ic<(STAGES > 3 ? 3 : 0)>{});
        };
        if (free_unclamped) run_my_stage(std::true_type{});
        else run_my_stage(std::false_type{});
        SOTS_PHASE(14); // the tile's samples are stored (issued)
    }
    if (table_pending) wavetable_ready(); // a workgroup without a tile must not end with copies in flight
    SOTS_PHASE_REAL(11);
}

// ------------------------------------------------------------------------------------
// Series voices: the OPERATORS in the lanes (k_synth_ol, round 4).
//
// k_synth gives an individual a lane, so a CU's share of 128 ... 256 individuals is two to four wavefronts - one per SIMD
// at best, and a wavefront alone on its SIMD issues an instruction every ~4.5 cycles where two or more sharing it issue
// one every ~2.3.  The cut kernels buy the second wavefront per SIMD with a wavefront per operator, LDS hand-overs and a
// workgroup barrier per 8 samples (4-op, 128 per CU: 24 of 89 busy LDS cycles per sample and 28 us of barrier).
// Here a LANE is one OPERATOR of one individual: a row of 16 lanes holds R = 8 / 4 / 4 individuals of the 2- / 3- / 4-operator
// voice, operator s of individual i in lane R s + i (3 operators: R (s + 1) + i, the lanes in front make operator 0's constant
// increment), so a wavefront carries 32 / 16 / 16 individuals and the CU's share is twice / four times as many wavefronts,
// every one of them running ONE instruction stream in which all 64 lanes work:
//   C  the lane's operator on its block of 8 samples: table read at the phase, phase += increment, wrap - the reference's
//      operations (operator 0's second wrap adds 0 instead of W: it has only the first, Evolutionary_Strategy.hpp:383,418);
//   A  the block read ONE TRIP AGO (its table values have landed): t * pm (for the last operator: the sample), + po, * c -
//      the next operator's increments c * (t * mul + off), unfused, two samples per packed instruction;
//   B  hand-over to the operator behind: ONE v_mov_b32_dpp row_shr:R per sample, no LDS, no barrier.  The bottom R lanes
//      of a row have no source lane; DPP leaves such lanes alone, so operator 0's registers keep c * p1, the free-running
//      operator's constant increment.
// Operator s works on block k - 2 s in trip k (its increments were handed over in trip k - 1 from table values read in
// trip k - 2).  The last operator's samples are spread over the G lanes of their individual (row_shl) so that every lane parks
// 32 / G bytes per trip in the wavefront's tile with ONE LDS instruction (a write instruction costs the LDS the same 6-13 cycles
// whether 16 lanes carry data or 64); rows = individuals, whole 128-byte lines leave every 32 samples as in k_synth.
// Per sample and lane ~9 vector instructions + 1 LDS gather.  Every sample sees the reference's operations in its order:
// bit-identical to k_synth and the oracle.
// What it reaches (profiles/r04_experiments.md; tools/ubench/ol_loop.hip, lds_gather.hip): 87 cycles per sample for the
// median wavefront and 97 for the slowest at configs[3]'s shard (k_synth<4OP, 1, ., 2, 3>: 112) - not the ~55 the LDS would
// allow (a random 64-lane gather costs it 4.8-5.9 cycles, eight per sample): a wavefront of this instruction mix (v_cvt, v_pk_*,
// three-operand integer minima, DPP moves at ~8 cycles each) needs 47-53 cycles per sample ALONE on its SIMD, a second one
// adds only ~30 % (the SIMD issues oldest-first: 54 / 78 in isolation, the kernel ends with the younger), so only the
// 4-operator voice at 65 ... 128 individuals per CU runs here (launch_synth).
// ------------------------------------------------------------------------------------
template <int OPS> struct OlShape {
    static constexpr int G = OPS == 2 ? 2 : 4; // lanes per individual (3 operators: a fourth lane in front of operator 0 supplies its constant increment)
    static constexpr int R = 16 / G;         // individuals per row of 16 lanes: 8 or 4
    static constexpr int IPW = 4 * R;        // individuals per wavefront: 32 or 16
    static constexpr int NI = IPW / 8;       // store instructions per flush (8 rows x 128 bytes each)
};
constexpr int kOlTileRows = 240; // individuals per workgroup at most: 240 x 128 bytes of tiles + the table's spare entry in the 32 KiB beside the table
template <int OPS> constexpr int ol_max_waves() { return kOlTileRows / OlShape<OPS>::IPW; } // 7 or 15

template <int KIND>
__global__ __launch_bounds__(ol_max_waves<VoiceShape<KIND>::OPS>() * kWave) void k_synth_ol(const float *__restrict__ values,
                                                               const float *__restrict__ wavetable,
                                                               float *__restrict__ audio, SynthParams sp,
                                                               uint32_t p_len, uint32_t n, uint32_t pitch, Variation var)
{
    constexpr int OPS = VoiceShape<KIND>::OPS, D = VoiceShape<KIND>::D;
    static_assert(VoiceShape<KIND>::J == 1, "series voices");
    constexpr int G = OlShape<OPS>::G, R = OlShape<OPS>::R, IPW = OlShape<OPS>::IPW, NI = OlShape<OPS>::NI;
#ifndef SOTS_OL_U
#define SOTS_OL_U 16
#endif
    // samples per trip: 16 where a lane is one of four per individual (the per-trip work - tile addresses, the flush test, loop and
    // priority bookkeeping - over twice the samples: 157 -> 146-150 us at configs[3]'s shard; 32 would not fit 128 registers), 8 for the 2-operator layout
#ifndef SOTS_OL_U2
#define SOTS_OL_U2 8
#endif
    constexpr int U = G == 4 ? SOTS_OL_U : SOTS_OL_U2, CH = kStageChunks;
    constexpr int LAST = 2 * OPS - 1; // the block whose samples leave in trip k is k - LAST
    __shared__ float tab[kWavetableSize + 64]; // entry W repeats entry W - 1: the clamp-free index below may reach it
    __shared__ float4 stage_all[kOlTileRows * CH + 4]; // the tiles + 64 bytes of progress counters
    request_wavetable(tab, wavetable);
    bool table_pending = true;
    const float c = (float)kWavetableSize / (float)SOTS_SAMPLE_RATE; // w2srRatio, Evolutionary_Strategy.hpp:203
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), waves = blockDim.x / kWave;
    const uint32_t lr = lane & 15u, grp = lr / (uint32_t)R;        // this lane's place among the G lanes of its individual
    const int s = (int)grp - (G - OPS);                            // ... i.e. its operator; -1: the 3-operator voice's constant source
    const uint32_t li = (lane >> 4) * R + (lr - grp * R);          // ... of which individual of the wavefront
    const uint32_t rows_per_block = waves * IPW;
    const uint32_t sharers = (waves + 3u) / 4u; // the wavefronts of a workgroup go to the SIMDs in turn: w, w + 4, ... share one
    float4 *__restrict__ stage = stage_all + wave * (IPW * CH);
    // write side: the last operator's samples are spread over the G lanes of their individual first (row shifts), so that
    // EVERY lane parks 32 / G bytes with one instruction; row = individual, chunk q in slot q ^ (row & 7)
    const uint32_t l7 = li & 7u;
    const uint32_t r8 = lane / CH, rch = lane % CH; // read side: lane = (row within a group of 8, chunk)
    const float4 *__restrict__ rd = stage + r8 * CH + (rch ^ (r8 & 7u));
    const uint32_t lane_off = r8 * pitch + 4u * rch;
    uint32_t row_off[NI];
#pragma unroll
    for (int g = 0; g < NI; ++g) row_off[g] = (lane_off + (uint32_t)g * 8u * pitch) * 4u; // bytes; < 2^32: 32 rows of at most 8224 floats

    // progress counters of the wavefronts (below): 64 bytes behind the workgroup's tiles
    int *__restrict__ progress = reinterpret_cast<int *>(stage_all + rows_per_block * CH);
    const bool feedback = sharers > 1u;
    const uint32_t first_base = blockIdx.x * rows_per_block;
    for (uint32_t base = first_base; base < p_len; base += gridDim.x * rows_per_block) {
        const uint32_t row0 = base + wave * IPW; // first row of this wavefront
        const uint32_t ind = row0 + li < p_len ? row0 + li : p_len - 1u;
        float p[D];
        if (var.vin) {
            // fused generation loop: the workgroup makes its individuals, a thread per gene (k_recombine_mutate's
            // arithmetic), writes them to the other half and leaves the values in LDS for the lanes that need them
            // (the tile area: nothing is parked there yet)
            float *__restrict__ made = reinterpret_cast<float *>(stage_all);
            if (base != first_base) __syncthreads(); // the previous tile's last lines have been read back
            for (uint32_t t = threadIdx.x; t < rows_per_block * D; t += blockDim.x) {
                const uint32_t i1 = base + t / D, g1 = t % D;
                if (i1 < p_len) {
                    float x, st;
                    make_gene(x, st, var.vin, var.sin, 0u, i1, g1, var.generation, var.pd, var.mc);
                    var.vout[(size_t)i1 * D + g1] = x;
                    var.sout[(size_t)i1 * D + g1] = st;
                    made[t] = x;
                }
            }
            __syncthreads();
#pragma unroll
            for (int g = 0; g < D; ++g) p[g] = made[(ind - base) * D + g];
            __syncthreads(); // everybody has its genes: the tiles may be written
        } else {
#pragma unroll
            for (int g = 0; g < D; ++g) p[g] = values[(size_t)ind * D + g];
        }
#pragma unroll
        for (int g = 0; g < D; ++g) p[g] = sp.pmin[g] + p[g] * (sp.pmax[g] - sp.pmin[g]); // scaleParams, ocl_program.cl:297
        // operator s hands (t * pm + po) * c to operator s + 1; the last operator's t * pm is the sample
        float inc0c, pm = 0.0f, po = 0.0f;
        if constexpr (KIND == SOTS_SYNTH_2OP) { // Evolutionary_Strategy.hpp:372-401
            inc0c = c * p[0];
            pm = s == 0 ? p[0] * p[1] : p[3], po = s == 0 ? p[2] : 0.0f;
        } else { // series, :407-445 (the 4-operator voice adds one more modulator stage)
            inc0c = c * p[1];
#pragma unroll
            for (int o = 0; o < OPS; ++o)
                if (s == o) pm = p[2 * o] * p[2 * o + 1], po = o + 1 < OPS ? p[2 * o + 3] : 0.0f;
        }
        // 3 operators: the lane in front of operator 0 makes (t * 0 + p1) * c = c * p1 for it, sample after sample
        if (G > OPS && s < 0) pm = 0.0f, po = p[1];
        const float wlo = s <= 0 ? 0.0f : kWf; // operator 0 has the first wrap only
        if (table_pending) {
            wavetable_ready();
            if (threadIdx.x == 0) tab[kWavetableSize] = tab[kWavetableSize - 1];
            __syncthreads();
            table_pending = false;
        }
        // The index needs no clamp while every phase stays inside [0, W]: operator 0's increment in [0, W) (first wrap only), and
        // every handed-over increment c (t pm + po) smaller than W in magnitude - |t| <= 1, so c (|pm| + |po|) < W suffices, whatever
        // the table says (the lanes run on past their last block and before their first: only bounds that hold for every table
        // value count).  A phase that the second wrap's addition rounds up to exactly W reads entry W = entry W - 1, which is what
        // the reference's clamp makes of it (tab_at).  The reference's own parameter box qualifies (0.743 (3520 x 8 + 3520) < 32768);
        // any lane out of bounds, or NaN, sends the wavefront down the clamped path.
        const bool hands_over = s >= 0 && s < OPS - 1;
        const bool lane_bounded = (!hands_over || c * (__builtin_fabsf(pm) + __builtin_fabsf(po)) < 0.999f * kWf) && inc0c >= 0.0f && inc0c < kWf;
        const bool unclamped = __all(lane_bounded);

        auto run = [&](auto unclamped_tag) {
        constexpr bool UNCLAMPED = decltype(unclamped_tag)::value;
        float pos = 0.0f;
        float inc[U];  // this lane's increments for the block it works on next (operator 0: the constant, never overwritten)
        float T[2][U]; // table values of the block of this trip's parity / of the trip before
#pragma unroll
        for (int u = 0; u < U; ++u) inc[u] = s == 0 ? inc0c : 0.0f, T[0][u] = 0.0f, T[1][u] = 0.0f;
        float pend[NI][4];
        float *__restrict__ pend_line = audio;
        bool pending = false;
        auto store_pending = [&]() {
            if (!pending) return;
            pending = false;
#pragma unroll
            for (int g = 0; g < NI; ++g) {
                if (row0 + 8u * g + r8 >= p_len) continue;
                asm volatile("" : "+v"(row_off[g]));
                *reinterpret_cast<float4 *>(reinterpret_cast<char *>(pend_line) + row_off[g]) = make_float4(pend[g][0], pend[g][1], pend[g][2], pend[g][3]);
            }
        };
        const uint32_t nb = n / U;
        // PHASE 1: the first trips (an operator idles, increments 0, until its first block arrives; samples leave from trip LAST),
        // 0: the body, 2: the last trips (samples leave while their block exists)
        auto trip = [&](auto q_tag, auto phase_tag, uint32_t k) {
            constexpr int Q = decltype(q_tag)::value, PHASE = decltype(phase_tag)::value;
            // C: this lane's operator on its block
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if constexpr (UNCLAMPED) {
                    T[Q][u] = tab[(uint32_t)pos]; // pos in [0, W]
                } else {
                    // table[clamp((int)pos, 0, W-1)] (tab_at): v_cvt_u32_f32 saturates - negative and NaN give 0, as the
                    // oracle's tab_at does - then one unsigned minimum; both cheaper to issue than the signed med3
                    uint32_t ti;
                    asm("v_cvt_u32_f32 %0, %1" : "=v"(ti) : "v"(pos));
                    T[Q][u] = tab[min(ti, kWavetableSize - 1u)];
                }
                pos += inc[u];
                const v2f_t bc = v2f_t{pos, pos} + v2f_t{-kWf, wlo};
                pos = __uint_as_float(min(min(__float_as_uint(bc.x), __float_as_uint(bc.y)), __float_as_uint(pos)));
            }
            // (nothing of A may move above this trip's table reads: it would wait for the reads of the trip before with none in
            // flight behind them - the scheduler did, and every trip began with s_waitcnt lgkmcnt(0))
            __builtin_amdgcn_sched_barrier(0);
            // A: the block read one trip ago (its table values have landed): t * pm (the last operator's samples), + po, * c
            v2f_t m[U / 2];
#pragma unroll
            for (int u = 0; u < U; u += 2) {
                m[u / 2] = v2f_t{T[Q ^ 1][u], T[Q ^ 1][u + 1]} * pm;
                const v2f_t o = (m[u / 2] + po) * c;
                // B: to the operator behind (lanes R ... 15 of every row take from R lanes below; lanes 0 ... R-1 have no source lane
                // and keep theirs: operator 0's constant)
                inc[u] = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(inc[u]), __float_as_int(o.x), 0x110 + R, 0xf, 0xf, false));
                inc[u + 1] = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(inc[u + 1]), __float_as_int(o.y), 0x110 + R, 0xf, 0xf, false));
            }
            if constexpr (PHASE == 1) {
                if (s >= 1 && 2u * (uint32_t)s > k + 1u) { // this operator's first block has not arrived yet
#pragma unroll
                    for (int u = 0; u < U; ++u) inc[u] = 0.0f;
                }
            }
            // the samples of block k - LAST leave
            if (PHASE == 0 || (k >= (uint32_t)LAST && k - (uint32_t)LAST < nb)) {
                const uint32_t ip = (k - (uint32_t)LAST) * U;
                store_pending(); // the lines read back one trip ago
                const uint32_t c0 = (ip >> 2) & (CH - 1);
                // the 8 samples sit in the last operator's lanes (the top R lanes of every row): lane group g of the individual takes
                // samples 8 g / G ... from them (row_shl: a lane reads the lane n above it; lanes without a source keep theirs), then
                // all 64 lanes write (a write instruction costs the LDS the same whether 16 lanes carry data or 64: 26 -> 6 cycles per sample and CU)
                auto shl = [&](float keep, float src, auto n_tag) {
                    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(keep), __float_as_int(src), 0x100 + decltype(n_tag)::value, 0xf, 0xf, false));
                };
                if constexpr (G == 4 && U == 16) { // 16-sample trips: a whole chunk of 16 bytes per lane
                    float4 w = make_float4(m[6].x, m[6].y, m[7].x, m[7].y);
                    w.x = shl(w.x, m[4].x, ic<R>{}), w.y = shl(w.y, m[4].y, ic<R>{}), w.z = shl(w.z, m[5].x, ic<R>{}), w.w = shl(w.w, m[5].y, ic<R>{});
                    w.x = shl(w.x, m[2].x, ic<2 * R>{}), w.y = shl(w.y, m[2].y, ic<2 * R>{}), w.z = shl(w.z, m[3].x, ic<2 * R>{}), w.w = shl(w.w, m[3].y, ic<2 * R>{});
                    w.x = shl(w.x, m[0].x, ic<3 * R>{}), w.y = shl(w.y, m[0].y, ic<3 * R>{}), w.z = shl(w.z, m[1].x, ic<3 * R>{}), w.w = shl(w.w, m[1].y, ic<3 * R>{});
                    stage[li * CH + ((c0 + grp) ^ l7)] = w;
                } else if constexpr (G == 4) {
                    v2f_t w = m[3];
                    w.x = shl(w.x, m[2].x, ic<R>{}), w.y = shl(w.y, m[2].y, ic<R>{});
                    w.x = shl(w.x, m[1].x, ic<2 * R>{}), w.y = shl(w.y, m[1].y, ic<2 * R>{});
                    w.x = shl(w.x, m[0].x, ic<3 * R>{}), w.y = shl(w.y, m[0].y, ic<3 * R>{});
                    float2 *__restrict__ wr2 = reinterpret_cast<float2 *>(stage + li * CH);
                    wr2[((c0 + (grp >> 1)) ^ l7) * 2u + (grp & 1u)] = make_float2(w.x, w.y);
                } else if constexpr (U == 16) { // two lanes per individual, 16-sample trips: two chunks per lane
                    float4 w0 = make_float4(m[4].x, m[4].y, m[5].x, m[5].y), w1 = make_float4(m[6].x, m[6].y, m[7].x, m[7].y);
                    w0.x = shl(w0.x, m[0].x, ic<R>{}), w0.y = shl(w0.y, m[0].y, ic<R>{}), w0.z = shl(w0.z, m[1].x, ic<R>{}), w0.w = shl(w0.w, m[1].y, ic<R>{});
                    w1.x = shl(w1.x, m[2].x, ic<R>{}), w1.y = shl(w1.y, m[2].y, ic<R>{}), w1.z = shl(w1.z, m[3].x, ic<R>{}), w1.w = shl(w1.w, m[3].y, ic<R>{});
                    stage[li * CH + ((c0 + 2u * grp) ^ l7)] = w0;
                    stage[li * CH + ((c0 + 2u * grp + 1u) ^ l7)] = w1;
                } else {
                    float4 w = make_float4(m[2].x, m[2].y, m[3].x, m[3].y);
                    w.x = shl(w.x, m[0].x, ic<R>{}), w.y = shl(w.y, m[0].y, ic<R>{}), w.z = shl(w.z, m[1].x, ic<R>{}), w.w = shl(w.w, m[1].y, ic<R>{});
                    stage[li * CH + ((c0 + grp) ^ l7)] = w;
                }
                if (c0 == CH - U / 4) { // 32 samples parked: the tile is read back transposed (LDS works in order) and stored in the next trip
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("" ::: "memory");
#pragma unroll
                    for (int g = 0; g < NI; ++g) {
                        const float4 q = rd[g * (8 * CH)];
                        pend[g][0] = q.x, pend[g][1] = q.y, pend[g][2] = q.z, pend[g][3] = q.w;
                    }
                    pend_line = audio + (size_t)row0 * pitch + (ip + U - 4 * CH); // wavefront-uniform
                    pending = true;
                    __builtin_amdgcn_wave_barrier();
                    asm volatile("" ::: "memory");
                }
            }
        };
        if (feedback && lane == 0) progress[wave] = 0; // (a stale count of the tile before only costs a priority)
        constexpr uint32_t K0 = 2 * OPS; // first trip (even) in which every operator works and samples leave
        SOTS_STAMP_SCOPE(blockIdx.x * (blockDim.x / kWave) + wave); // (diagnostic builds: this wavefront's cycles over all trips)
        for (uint32_t k = 0; k < K0; k += 2) {
            trip(ic<0>{}, ic<1>{}, k);
            trip(ic<1>{}, ic<1>{}, k + 1);
        }
        for (uint32_t k = K0; k < nb; k += 2) {
#ifndef SOTS_OL_NO_FEEDBACK
            // The SIMD issues for its OLDEST wavefront first: of two that share it the older runs as if alone (54 cycles per sample in
            // isolation) and the younger takes what is left (78) - and the kernel ends with the younger.  Every 16 trips a wavefront
            // publishes its trip count in LDS and takes priority = the number of wavefronts sharing its SIMD (w, w + 4, ... of the
            // workgroup) that are AHEAD of it, so the laggard issues first: 70 / 71 in isolation (tools/ubench/ol_loop.hip).
            // (Priority TURNS - a trip each, or 32 - even the two out at the slow end; s_setprio takes an immediate, hence the branches.)
            if (feedback && (k & 15u) == 0u) {
                if (lane == 0) __hip_atomic_store(&progress[wave], (int)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                uint32_t ahead = 0;
                for (uint32_t q = 1; q < sharers; ++q) {
                    const uint32_t other = (wave + 4u * q) % (4u * sharers);
                    ahead += other < waves && __hip_atomic_load(&progress[other], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > (int)k ? 1u : 0u;
                }
                ahead = __builtin_amdgcn_readfirstlane(ahead);
                asm volatile("s_cmp_eq_u32 %0, 0\n\ts_cbranch_scc1 10f\n\ts_cmp_eq_u32 %0, 1\n\ts_cbranch_scc1 11f\n\ts_cmp_eq_u32 %0, 2\n\ts_cbranch_scc1 12f\n\t"
                             "s_setprio 3\n\ts_branch 19f\n10:\ts_setprio 0\n\ts_branch 19f\n11:\ts_setprio 1\n\ts_branch 19f\n12:\ts_setprio 2\n19:" ::"s"(ahead) : "scc");
            }
#endif
            trip(ic<0>{}, ic<0>{}, k);
            trip(ic<1>{}, ic<0>{}, k + 1);
        }
        for (uint32_t k = nb; k < nb + K0; k += 2) { // the last block leaves in trip nb - 1 + LAST
            trip(ic<0>{}, ic<2>{}, k);
            trip(ic<1>{}, ic<2>{}, k + 1);
        }
        store_pending();
        };
        if (unclamped) run(std::true_type{});
        else run(std::false_type{});
    }
    if (table_pending) wavetable_ready(); // a workgroup without a tile must not end with copies in flight
}

// ------------------------------------------------------------------------------------
// SMALL populations (a few individuals per CU), every voice: the time axis in the lanes.
//
// k_synth above puts an individual in a lane and pays its ten to twenty vector instructions per sample and operator whether
// one lane is alive or sixty-four; with a few individuals per CU almost all of that is arithmetic on dead lanes.  But only the
// PHASE of an operator is a recurrence over the samples - pos[n+1] = wrap(pos[n] + inc[n]), three dependent instructions -
// while everything else (the table read at pos[n], t mul + off, times c, times the gain) is independent per sample.  So
// operator s has TWO wavefronts here, and per block of 64 samples
//   * its SCAN wavefront, lane = individual, reads the 64 increments of its individual (operator 0: a constant) and writes
//     the 64 phases in their place - the reference's additions and wraps, in its order;
//   * its EVALUATION wavefront, lane = SAMPLE, takes individual after individual: table value at the phase, then either the
//     next operator's increment c (t mul + off) into that operator's buffer or gain t to the audio row (a whole 256-byte
//     piece of a row per instruction).
// A pipeline of 2 OPS stages, one block and one workgroup barrier per tick, three buffers per operator in rotation (the
// evaluation of block b reads a buffer in the tick in which block b + 2's increments are written).  Every sample sees exactly the
// reference's operations, unfused: bit-identical to k_synth and the oracle.  What is left per sample is the latency of the
// three dependent instructions of a scan (~30 cycles; k_synth: ~90): profiles/r03_experiments.md.
// ------------------------------------------------------------------------------------
constexpr int kTpRow = 64 + 4; // floats per (individual, block) row: the scan's 16-byte accesses of neighbouring lanes on different banks
// individuals per workgroup: three rows per operator each (and, for the voice of three parallel chains, two rows for each of
// the two products that wait for the third), in the 31 KiB beside the table that the genes leave: 19 / 12 / 9 for 2, 3, 4
// operators in series (populations up to 4864 / 3072 / 2304 on 256 CUs), 5 for the triple voice (1280)
template <int KIND> constexpr int tp_max_individuals()
{
    return (31 * 1024) / ((VoiceShape<KIND>::J * VoiceShape<KIND>::OPS * 3 + (VoiceShape<KIND>::J > 1 ? 2 * (VoiceShape<KIND>::J - 1) : 0)) * kTpRow * 4);
}

// evaluating wavefronts per operator: two for the series voices (from about eight individuals per CU the evaluation of a
// block takes longer than its scan: the two take every other batch of four), one for the triple voice (six operators)
template <int KIND> constexpr int tp_eval_waves() { return VoiceShape<KIND>::J == 1 ? 2 : 1; }
template <int KIND> constexpr int tp_waves() { return VoiceShape<KIND>::J * VoiceShape<KIND>::OPS * (1 + tp_eval_waves<KIND>()); }

template <int KIND>
__global__ __launch_bounds__(tp_waves<KIND>() * kWave) void k_synth_tp(const float *__restrict__ values,
                                                                                const float *__restrict__ wavetable,
                                                                                float *__restrict__ audio, SynthParams sp,
                                                                                uint32_t p_len, uint32_t n, uint32_t pitch,
                                                                                uint32_t per_group, Variation var)
{
    // J > 1 (the voice of three 2-operator chains, averaged): every chain has its own pipeline; chains 1 ... J-1 leave gain t
    // in LDS and chain 0, which runs one tick behind them, adds the products in the reference's order and divides
    constexpr int J = VoiceShape<KIND>::J, OPS = VoiceShape<KIND>::OPS, D = VoiceShape<KIND>::D, IMAX = tp_max_individuals<KIND>();
    constexpr int NE = tp_eval_waves<KIND>();
    constexpr uint32_t THREADS = tp_waves<KIND>() * kWave;
    __shared__ float tab[kWavetableSize];
    __shared__ __attribute__((aligned(16))) float buf[J * OPS][3][IMAX][kTpRow]; // [chain, operator][block mod 3][individual][sample]: increments, then phases
    __shared__ float prod[J > 1 ? J - 1 : 1][2][J > 1 ? IMAX : 1][J > 1 ? kTpRow : 1]; // [chain - 1][block parity]: gain t of chains 1 ... J-1
    __shared__ float made[IMAX * D];
    request_wavetable(tab, wavetable);
    const float c = (float)kWavetableSize / (float)SOTS_SAMPLE_RATE; // w2srRatio, Evolutionary_Strategy.hpp:203
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const int wave = (int)__builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const bool scans = wave < J * OPS; // the first J OPS wavefronts scan, the others evaluate (NE per operator)
    const int jo = scans ? wave : (wave - J * OPS) / NE, jc = jo / OPS, s = jo % OPS; // this wavefront's chain and operator
    const uint32_t ev = scans ? 0u : (uint32_t)((wave - J * OPS) % NE);                // ... and which of its evaluators
    const uint32_t first = blockIdx.x * per_group;
    const uint32_t count = first >= p_len ? 0u : (p_len - first < per_group ? p_len - first : per_group); // individuals here (<= IMAX)

    // the individuals: read, or made here (fused generation loop: one gene per thread)
    if (var.vin) {
        for (uint32_t t = threadIdx.x; t < count * D; t += THREADS) {
            const uint32_t i1 = first + t / D, g1 = t % D;
            float x, st;
            make_gene(x, st, var.vin, var.sin, 0u, i1, g1, var.generation, var.pd, var.mc);
            var.vout[(size_t)i1 * D + g1] = x;
            var.sout[(size_t)i1 * D + g1] = st;
            made[t] = x;
        }
    } else {
        for (uint32_t t = threadIdx.x; t < count * D; t += THREADS) made[t] = values[(size_t)first * D + t];
    }
    __syncthreads();
    // lane i < count: individual first + i.  scaleParams and the per-operator constants as in k_synth
    float pr[D];
#pragma unroll
    for (int g = 0; g < D; ++g) {
        pr[g] = lane < count ? made[lane * D + g] : 0.0f;
        const int sc = KIND == SOTS_SYNTH_TRIPLE_PAR ? (g & 3) : g; // the triple voice scales all three chains by entries 0..3, Evolutionary_Strategy.hpp:453-455
        pr[g] = sp.pmin[sc] + pr[g] * (sp.pmax[sc] - sp.pmin[sc]); // min + v*(max-min), ocl_program.cl:297
    }
    float inc0, mul_next = 0.0f, off_next = 0.0f, gain; // mul / off: what the evaluation of operator s applies for operator s + 1
    if constexpr (KIND == SOTS_SYNTH_2OP) { // Evolutionary_Strategy.hpp:372-401
        inc0 = c * pr[0];
        if (s == 0) mul_next = pr[0] * pr[1], off_next = pr[2];
        gain = pr[3];
    } else if constexpr (KIND == SOTS_SYNTH_TRIPLE_PAR) { // :457-494
        inc0 = 0.0f, gain = 0.0f;
#pragma unroll
        for (int jj = 0; jj < J; ++jj)
            if (jc == jj) {
                inc0 = c * pr[4 * jj], gain = pr[4 * jj + 3];
                if (s == 0) mul_next = pr[4 * jj] * pr[4 * jj + 1], off_next = pr[4 * jj + 2];
            }
    } else { // series, :407-445 (the 4-operator voice adds one more modulator stage)
        inc0 = c * pr[1];
#pragma unroll
        for (int o = 1; o < OPS; ++o)
            if (s == o - 1) mul_next = pr[2 * (o - 1)] * pr[2 * (o - 1) + 1], off_next = pr[2 * (o - 1) + 3];
        gain = pr[2 * (OPS - 1)] * pr[2 * (OPS - 1) + 1];
    }
    wavetable_ready();

    const uint32_t blocks = n / kWave;
    float pos = 0.0f; // (scan wavefronts) this operator's phase of individual `lane`
    constexpr uint32_t LAG0 = J > 1 ? 1u : 0u; // chain 0 of a parallel voice: one tick behind the others
    for (uint32_t tick = 0; tick < blocks + 2 * OPS - 1 + LAG0; ++tick) {
        // scan of operator s: block tick - 2 s; its evaluation: one tick later
        const uint32_t k = tick - 2u * (uint32_t)s - (scans ? 0u : 1u) - (jc == 0 ? LAG0 : 0u);
        if (k < blocks) {
            float(*rows)[kTpRow] = buf[jo][k % 3u];
            if (scans) {
                if (lane < count) { // lane = individual: phases in place of increments, four samples per access
                    float4 *row = reinterpret_cast<float4 *>(rows[lane]);
                    if (s == 0) {
#pragma unroll
                        for (int q = 0; q < kWave / 4; ++q) {
                            float4 o;
                            o.x = pos, pos += inc0, wrap_hi(pos);
                            o.y = pos, pos += inc0, wrap_hi(pos);
                            o.z = pos, pos += inc0, wrap_hi(pos);
                            o.w = pos, pos += inc0, wrap_hi(pos);
                            row[q] = o;
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < kWave / 4; ++q) {
                            const float4 v = row[q];
                            float4 o;
                            o.x = pos, pos += v.x, wrap_both(pos);
                            o.y = pos, pos += v.y, wrap_both(pos);
                            o.z = pos, pos += v.z, wrap_both(pos);
                            o.w = pos, pos += v.w, wrap_both(pos);
                            row[q] = o;
                        }
                    }
                }
            } else { // lane = sample
                const uint32_t sample = k * kWave + lane;
                // four individuals at a time: their phases, then their table values, are asked for together
                float(*next)[kTpRow] = buf[s + 1 < OPS ? jo + 1 : 0][k % 3u];
                for (uint32_t i0 = 4u * ev; i0 < count; i0 += 4u * NE) {
                    float ph[4], t[4];
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) ph[j] = rows[i0 + j < count ? i0 + j : i0][lane];
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) t[j] = tab_at<true>(tab, ph[j]);
#pragma unroll
                    for (uint32_t j = 0; j < 4; ++j) {
                        const uint32_t i = i0 + j;
                        if (i >= count) break;
                        if (s < OPS - 1) {
                            const float m = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mul_next), (int)i));
                            const float o = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(off_next), (int)i));
                            next[i][lane] = c * (t[j] * m + o); // the next operator's increment, unfused
                        } else {
                            const float g = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gain), (int)i));
                            if constexpr (J == 1) audio[(size_t)(first + i) * pitch + sample] = g * t[j];
                            else if (jc != 0) prod[jc - 1][k & 1u][i][lane] = g * t[j];
                            else // the reference's sum, in its order, and its division (== (float)(double(sum) / 3.0), :493)
                                audio[(size_t)(first + i) * pitch + sample] = (g * t[j] + prod[0][k & 1u][i][lane] + prod[J > 2 ? 1 : 0][k & 1u][i][lane]) / 3.0f;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------
// applyWindowPopulation, ocl_program.cl:566-586.  The table is the reference's double
// window (Evolutionary_Strategy.hpp:308-317) rounded once to fp32.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_window(float *__restrict__ audio, const float *__restrict__ window,
                                                size_t total4, uint32_t log2n4, uint32_t pitch4)
{
    float4 *a4 = reinterpret_cast<float4 *>(audio);
    const float4 *w4 = reinterpret_cast<const float4 *>(window);
    const uint32_t mask = (1u << log2n4) - 1u;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total4;
         e += (size_t)gridDim.x * blockDim.x) {
        const size_t row = e >> log2n4;
        const uint32_t col = (uint32_t)e & mask;
        float4 v = a4[row * pitch4 + col];
        const float4 w = w4[col];
        v.x *= w.x; v.y *= w.y; v.z *= w.z; v.w *= w.w;
        a4[row * pitch4 + col] = v;
    }
}

} // namespace
} // namespace sots

#include "kernels/fft.h"
#include "kernels/objective.h"
#include "kernels/sel_keys.h"
#include "kernels/spectral_wave.h"
#include "kernels/sort.h"
#include "kernels/select_tiles.h"
#include "kernels/select_splitters.h"
#include "kernels/spectral_x.h"
#include "kernels/spectral_big.h"

namespace sots {
namespace {

// ------------------------------------------------------------------------------------
// island exchange: rows of [fitness, values, steps]
// ------------------------------------------------------------------------------------
__global__ void k_pack_rows(const float *__restrict__ values, const float *__restrict__ steps,
                            const float *__restrict__ fitness, float *__restrict__ rows,
                            uint32_t first_row, uint32_t n_rows, uint32_t d)
{
    const uint32_t w = 2 * d + 1, total = n_rows * w;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t r = e / w, c = e - r * w, src = first_row + r;
        rows[e] = c == 0 ? fitness[src] : c <= d ? values[src * d + (c - 1)] : steps[src * d + (c - 1 - d)];
    }
}

// rows [skip_first, skip_first + skip_count) of the source are passed over (an island's own
// block inside an all-gathered buffer)
__global__ void k_unpack_rows(float *__restrict__ values, float *__restrict__ steps,
                              float *__restrict__ fitness, const float *__restrict__ rows,
                              uint32_t first_row, uint32_t n_rows, uint32_t d, uint32_t skip_first,
                              uint32_t skip_count)
{
    const uint32_t w = 2 * d + 1, total = n_rows * w;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t r = e / w, c = e - r * w, dst = first_row + r;
        const uint32_t sr = r < skip_first ? r : r + skip_count;
        const float v = rows[sr * w + c];
        if (c == 0) fitness[dst] = v;
        else if (c <= d) values[dst * d + (c - 1)] = v;
        else steps[dst * d + (c - 1 - d)] = v;
    }
}

inline uint32_t grid_for(uint64_t work, uint32_t threads, uint32_t cap = 2048)
{
    uint64_t g = (work + threads - 1) / threads;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (uint32_t)g;
}

} // namespace

// ------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------
hipError_t launch_init_population(hipStream_t st, float *values, float *steps, float *fitness,
                                  const PopDims &pd, uint32_t chunk)
{
    k_init_population<<<grid_for((uint64_t)pd.p * pd.d, 256), 256, 0, st>>>(values, steps, fitness, pd, chunk);
    return hipGetLastError();
}

hipError_t launch_recombine(hipStream_t st, const float *vin, const float *sin, float *vout, float *sout,
                            const PopDims &pd)
{
    k_recombine<<<grid_for((uint64_t)pd.p * pd.d, 256), 256, 0, st>>>(vin, sin, vout, sout, pd);
    return hipGetLastError();
}

hipError_t launch_mutate(hipStream_t st, float *values, float *steps, const PopDims &pd,
                         const MutateConsts &mc, uint32_t generation)
{
    k_mutate<<<grid_for((uint64_t)pd.p * pd.d, 256), 256, 0, st>>>(values, steps, pd, mc, generation);
    return hipGetLastError();
}

hipError_t launch_recombine_mutate(hipStream_t st, const float *vin, const float *sin, float *vout,
                                   float *sout, const PopDims &pd, const MutateConsts &mc,
                                   uint32_t generation)
{
    k_recombine_mutate<<<grid_for((uint64_t)pd.p * pd.d, 256), 256, 0, st>>>(vin, sin, vout, sout, pd, mc,
                                                                               generation);
    return hipGetLastError();
}

// Where k_synth_tp runs: at most 16 individuals per CU for the 2-operator voice (populations up to 4096; 22-27 us of
// synthesis against 32-35 at N = 1024; beyond that k_synth's cut kernels win), 12 / 9 / 5 for 3 / 4 operators in series /
// three parallel chains (what fits beside the table)
#ifndef SOTS_TP_2OP_MAX
#define SOTS_TP_2OP_MAX 16
#endif
#ifndef SOTS_OL_MIN_SHARE
#define SOTS_OL_MIN_SHARE 48
#endif
// Where k_synth_ol runs (same-box A/Bs, profiles/r04_experiments.md): the 4-operator voice from 65 individuals per CU (65 ... 240
// in one tile: 128 per CU 146-157 against 189 us, 192 per CU 199 against 297; beyond that in equal tiles: 256 per CU 302-307 against 313-317 + the
// variation launch, 313 per CU 389 against 612), the 3-operator voice at 65 ... 240 (128 per CU 91 against 95, 192 per CU 106 against
// 128; at 256 and 512 per CU k_synth wins: 126 against 152, 254 against 310)
bool synth_operators_in_lanes(uint32_t kind, uint32_t p, uint32_t num_cus)
{
#ifdef SOTS_SYNTH_NO_OL
    return false;
#else
    const uint32_t cus = num_cus ? num_cus : 256u, share = (p + cus - 1) / cus;
    if (kind == SOTS_SYNTH_4OP_SERIES) return share > 64u;
    if (kind == SOTS_SYNTH_3OP_SERIES) return share > 64u && share <= (uint32_t)kOlTileRows;
    return false;
#endif
}
bool synth_time_parallel(uint32_t kind, uint32_t p, uint32_t num_cus)
{
#ifdef SOTS_SYNTH_NO_TP
    return false;
#else
    const uint32_t share = (p + (num_cus ? num_cus : 256u) - 1) / (num_cus ? num_cus : 256u);
    switch (kind) {
    case SOTS_SYNTH_2OP: return share <= (uint32_t)SOTS_TP_2OP_MAX;
    case SOTS_SYNTH_3OP_SERIES: return share <= (uint32_t)tp_max_individuals<SOTS_SYNTH_3OP_SERIES>();
    case SOTS_SYNTH_4OP_SERIES: return share <= (uint32_t)tp_max_individuals<SOTS_SYNTH_4OP_SERIES>();
    case SOTS_SYNTH_TRIPLE_PAR: return share <= (uint32_t)tp_max_individuals<SOTS_SYNTH_TRIPLE_PAR>();
    default: return false;
    }
#endif
}

// ------------------------------------------------------------------------------------
// The voices with the arithmetic of the reference's DEVICE kernels (sots_set_synth_arithmetic, SOTS_ARITH_DEVICE_KERNELS):
// ocl_program.cl:280-443 writes the sample-rate ratio as the double expression (WAVETABLE_SIZE / 44100.0), so an increment
// is a double product rounded to float once (:308, :356, :417) and a modulated phase advances by a double multiply-add
// rounded once (:319, :364, :368, :425); the float multiply-adds are fused by the OpenCL build; the 3-op voice's second
// offset is params[4] (:363); the first phase of the 2-op and triple voices has no lower wrap (:322-323); the index is the
// bare conversion, so a phase that lands on W reads entry W (here: 0 = sin 2 pi, the table's own continuation).
// tests/test_ocl_reference.py holds the outputs of those kernels - compiled as they stand and run on this GPU - and this
// kernel reproduces them bit for bit.  A compatibility path (a lane per individual, samples through a 64 x 16 tile so that
// four lanes store one row's 64 bytes): nothing of BASELINE's configurations runs here.
// ------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void k_synth_dev(const float *__restrict__ values, const float *__restrict__ wavetable,
                                                   float *__restrict__ audio, SynthParams sp, uint32_t p_len, uint32_t n, uint32_t pitch)
{
    constexpr int D = VoiceShape<KIND>::D, U = 16, STRIDE = U + 1;
    static_assert(KIND != SOTS_SYNTH_4OP_SERIES, "the reference has no device kernel for the build-defined 4-op voice");
    __shared__ float tab[kWavetableSize + 1];
    __shared__ float tile_all[4][kWave * STRIDE];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (uint32_t i = tid; i < kWavetableSize; i += 256) tab[i] = wavetable[i];
    if (tid == 0) tab[kWavetableSize] = 0.0f;
    const uint32_t row = blockIdx.x * 256u + tid;
    const bool live = row < p_len;
    float ps[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const int s = KIND == SOTS_SYNTH_TRIPLE_PAR ? (i & 3) : i; // (one set of bounds for the three voices, as everywhere in this library)
        ps[i] = __builtin_fmaf(live ? values[(size_t)row * D + i] : 0.0f, sp.pmax[s] - sp.pmin[s], sp.pmin[s]);
    }
    const double cd = (double)kWavetableSize / 44100.0;
    auto at = [&](float pos) -> float {
        uint32_t i = pos > 0.0f ? (uint32_t)pos : 0u;
        return tab[i > kWavetableSize ? kWavetableSize : i];
    };
    auto advance = [&](float pos, float cur) -> float { return (float)__builtin_fma(cd, (double)cur, (double)pos); };
    auto wrap_hi = [&](float &pos) { if (pos >= kWf) pos -= kWf; };
    auto wrap_lo = [&](float &pos) { if (pos < 0.0f) pos += kWf; };
    constexpr int J = KIND == SOTS_SYNTH_TRIPLE_PAR ? 3 : 1;
    float pa[J] = {}, pb[J] = {}, pc = 0.0f, inc[J], mod[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        mod[j] = ps[4 * j + 0] * ps[4 * j + 1];
        inc[j] = (float)(cd * (double)ps[KIND == SOTS_SYNTH_3OP_SERIES ? 1 : 4 * j]);
    }
    const float m2 = KIND == SOTS_SYNTH_3OP_SERIES ? ps[2] * ps[3] : 0.0f, m3 = KIND == SOTS_SYNTH_3OP_SERIES ? ps[D - 2] * ps[D - 1] : 0.0f;
    float *const tile = tile_all[wave];
    __syncthreads();
    for (uint32_t s0 = 0; s0 < n; s0 += U) {
#pragma unroll 4
        for (int u = 0; u < U; ++u) {
            float out;
            if constexpr (KIND == SOTS_SYNTH_3OP_SERIES) {
                const float cur1 = __builtin_fmaf(at(pa[0]), mod[0], ps[3]);
                pa[0] += inc[0];
                const float cur2 = __builtin_fmaf(at(pb[0]), m2, ps[4]);
                pb[0] = advance(pb[0], cur1);
                out = at(pc) * m3;
                pc = advance(pc, cur2);
                wrap_hi(pa[0]), wrap_lo(pa[0]), wrap_hi(pb[0]), wrap_lo(pb[0]), wrap_hi(pc), wrap_lo(pc);
            } else {
                float tot[J];
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const float cur = __builtin_fmaf(at(pa[j]), mod[j], ps[4 * j + 2]);
                    tot[j] = at(pb[j]) * ps[4 * j + 3];
                    pa[j] += inc[j];
                    pb[j] = advance(pb[j], cur);
                    wrap_hi(pa[j]), wrap_hi(pb[j]), wrap_lo(pb[j]);
                }
                if constexpr (J == 3) out = (float)((double)(tot[0] + tot[1] + tot[2]) / 3.0);
                else out = tot[0];
            }
            tile[lane * STRIDE + u] = out;
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < 4; ++it) { // four lanes per row: 64 contiguous bytes
            const uint32_t r = it * 16u + lane / 4u, c = (lane & 3u) * 4u;
            const uint32_t grow = blockIdx.x * 256u + wave * kWave + r;
            const float4 v = make_float4(tile[r * STRIDE + c], tile[r * STRIDE + c + 1], tile[r * STRIDE + c + 2], tile[r * STRIDE + c + 3]);
            if (grow < p_len) *reinterpret_cast<float4 *>(audio + (size_t)grow * pitch + s0 + c) = v;
        }
        __syncthreads();
    }
}

hipError_t launch_synth_device_arith(hipStream_t st, uint32_t kind, const float *values, const float *wavetable, float *audio,
                                     const SynthParams &sp, uint32_t p, uint32_t log2n, uint32_t pitch)
{
    const uint32_t n = 1u << log2n, grid = (p + 255u) / 256u;
    switch (kind) {
    case SOTS_SYNTH_2OP: k_synth_dev<SOTS_SYNTH_2OP><<<grid, 256, 0, st>>>(values, wavetable, audio, sp, p, n, pitch); break;
    case SOTS_SYNTH_3OP_SERIES: k_synth_dev<SOTS_SYNTH_3OP_SERIES><<<grid, 256, 0, st>>>(values, wavetable, audio, sp, p, n, pitch); break;
    case SOTS_SYNTH_TRIPLE_PAR: k_synth_dev<SOTS_SYNTH_TRIPLE_PAR><<<grid, 256, 0, st>>>(values, wavetable, audio, sp, p, n, pitch); break;
    default: return hipErrorInvalidValue; // (the 4-op voice is build-defined: the reference has no kernel to agree with)
    }
    return hipGetLastError();
}

hipError_t launch_synth(hipStream_t st, uint32_t kind, const float *values, const float *wavetable,
                        float *audio, const SynthParams &sp, uint32_t p, uint32_t log2n, uint32_t pitch,
                        uint32_t num_cus, const Variation *variation, bool allow_cut, const sots_voice_graph *graph,
                        uint32_t waveforms, const float *feedback, uint32_t feedback_genes)
{
    // the operator-graph voice has one kernel form, in a file of its own; it makes no individuals
    if (kind == SOTS_SYNTH_GRAPH) {
        if (!graph || variation) return hipErrorInvalidValue;
        return launch_synth_graph(st, *graph, values, wavetable, audio, sp, p, log2n, pitch, num_cus, waveforms, feedback, feedback_genes);
    }
    Variation var = {};
    if (variation) var = *variation;
    const uint32_t n = 1u << log2n;
    const uint32_t cus = num_cus ? num_cus : 256;
    // The 128 KiB table allows one workgroup per CU, so the workgroup is sized to the CU's share
    // of the population, up to one wavefront per SIMD; larger populations loop.  Up to two
    // wavefronts' worth per CU, a series voice is cut into two wavefronts per 64 individuals.
    const uint32_t share = (p + cus - 1) / cus;
    // a few individuals per CU: the time axis in the lanes (k_synth_tp), two wavefronts per operator
    if (allow_cut && synth_time_parallel(kind, p, num_cus)) {
        switch (kind) {
        case SOTS_SYNTH_2OP: k_synth_tp<SOTS_SYNTH_2OP><<<(p + share - 1) / share, tp_waves<SOTS_SYNTH_2OP>() * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, share, var); break;
        case SOTS_SYNTH_3OP_SERIES: k_synth_tp<SOTS_SYNTH_3OP_SERIES><<<(p + share - 1) / share, tp_waves<SOTS_SYNTH_3OP_SERIES>() * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, share, var); break;
        case SOTS_SYNTH_TRIPLE_PAR: k_synth_tp<SOTS_SYNTH_TRIPLE_PAR><<<(p + share - 1) / share, tp_waves<SOTS_SYNTH_TRIPLE_PAR>() * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, share, var); break;
        default: k_synth_tp<SOTS_SYNTH_4OP_SERIES><<<(p + share - 1) / share, tp_waves<SOTS_SYNTH_4OP_SERIES>() * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, share, var); break;
        }
        return hipGetLastError();
    }
    // The 3- and 4-operator voices from 65 individuals per CU (BASELINE configs[3]'s shard: 128): the operators in the lanes
    // (k_synth_ol; where exactly: synth_operators_in_lanes above) - every wavefront carries 16 individuals, up to fifteen wavefronts per
    // CU without hand-overs or barriers.  The 2-operator voice stays on k_synth (224 per CU: 49.3 against 51.1 us, and 256 per CU - BASELINE
    // configs[2] - leaves no LDS for the spare table entry and the progress counters); `SOTS_OL_ALL` is an experiment switch.
#ifndef SOTS_SYNTH_NO_OL
#ifdef SOTS_OL_ALL
    const bool use_ol = allow_cut && kind != SOTS_SYNTH_TRIPLE_PAR && share >= (uint32_t)SOTS_OL_MIN_SHARE;
#else
    const bool use_ol = allow_cut && synth_operators_in_lanes(kind, p, num_cus);
#endif
    if (use_ol) {
        auto launch_ol = [&](auto kind_tag) {
            constexpr int K = decltype(kind_tag)::value, OPS = VoiceShape<K>::OPS, IPW = OlShape<OPS>::IPW;
            constexpr uint32_t max_rows = ol_max_waves<OPS>() * IPW;
            // a CU's share in equal tiles of at most max_rows rows (256 per CU: two tiles of 128, not 240 + 16)
            const uint32_t tiles_per_cu = (share + max_rows - 1) / max_rows;
            uint32_t rows = ((share + tiles_per_cu - 1) / tiles_per_cu + IPW - 1) / IPW * IPW;
            rows = rows > max_rows ? max_rows : rows;
            uint32_t grid = (p + rows - 1) / rows;
            grid = grid > cus ? cus : grid; // larger populations: a workgroup takes several tiles
            k_synth_ol<K><<<grid, rows / IPW * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        };
        switch (kind) {
        case SOTS_SYNTH_2OP: launch_ol(ic<SOTS_SYNTH_2OP>{}); break;
        case SOTS_SYNTH_3OP_SERIES: launch_ol(ic<SOTS_SYNTH_3OP_SERIES>{}); break;
        default: launch_ol(ic<SOTS_SYNTH_4OP_SERIES>{}); break;
        }
        return hipGetLastError();
    }
#endif
    uint32_t waves = (share + kWave - 1) / kWave;
    waves = waves < 1 ? 1 : waves > (uint32_t)kSynthWaves ? (uint32_t)kSynthWaves : waves;
    const bool cut = allow_cut && waves <= 2 && kind != SOTS_SYNTH_TRIPLE_PAR;
    const uint32_t threads = (cut ? 2 : 1) * waves * kWave, grid = grid_for(p, waves * kWave, cus);
    // variation folded in, 2-operator voice, full workgroups with one tile each: sixteen wavefronts make the individuals
    if (var.vin && kind == SOTS_SYNTH_2OP && !cut && (uint64_t)grid * waves * kWave * 2 >= p) { // one or two tiles per workgroup
        k_synth<SOTS_SYNTH_2OP, 0, true><<<grid, 4 * waves * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        return hipGetLastError();
    }
    // ... and the cut kernels of a small population likewise: four threads per individual make the genes (one, two or three
    // each), then a wavefront per stage and 64 individuals stays (one tile per workgroup there)
    if (var.vin && cut && (uint64_t)grid * waves * kWave >= p) {
        const uint32_t ht = 4 * waves * kWave;
        switch (kind) {
        case SOTS_SYNTH_2OP: k_synth<SOTS_SYNTH_2OP, 1, true><<<grid, ht, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var); return hipGetLastError();
        // up to 64 individuals per CU every operator of a 3- or 4-operator chain gets a wavefront of its own (three or four
        // SIMDs busy; a stage is one operator long: 3-op N = 2048 P = 1024 105 -> 81 us per generation, 4-op N = 4096 204 -> 170)
        case SOTS_SYNTH_3OP_SERIES:
            if (waves == 1) k_synth<SOTS_SYNTH_3OP_SERIES, 1, true, 2><<<grid, ht, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
            else k_synth<SOTS_SYNTH_3OP_SERIES, 2, true><<<grid, ht, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
            return hipGetLastError();
        case SOTS_SYNTH_4OP_SERIES:
            if (waves == 1) k_synth<SOTS_SYNTH_4OP_SERIES, 1, true, 2, 3><<<grid, ht, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
            else k_synth<SOTS_SYNTH_4OP_SERIES, 1, true, 2, 3><<<grid, ht, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var); // (all eight wavefronts stay)
            return hipGetLastError();
        default: break;
        }
    }
#define SOTS_SYNTH_CASE(K, S)                                                                            \
    case K:                                                                                              \
        if (cut) k_synth<K, S><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var); \
        else k_synth<K, 0><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);     \
        break;
    switch (kind) {
        SOTS_SYNTH_CASE(SOTS_SYNTH_2OP, 1)
    case SOTS_SYNTH_3OP_SERIES:
        // one group of 64 per CU: a wavefront per operator (three SIMDs); two groups: the chain cut once (four wavefronts)
        if (cut && waves == 1) k_synth<SOTS_SYNTH_3OP_SERIES, 1, false, 2><<<grid, 3 * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        else if (cut) k_synth<SOTS_SYNTH_3OP_SERIES, 2><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        else k_synth<SOTS_SYNTH_3OP_SERIES, 0><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        break;
    case SOTS_SYNTH_4OP_SERIES:
        // up to 128 individuals per CU a wavefront per operator: four wavefronts for one group of 64 (round 2: three stages
        // {0, 1} | {2} | {3} with 16-sample blocks: 165 against 131 us at P = 1024, N = 4096), eight for two (BASELINE configs[3]'s
        // shard; `-DSOTS_SYNTH_NO_CUT3`: the single cut of round 2 there)
#ifndef SOTS_SYNTH_NO_CUT3
        if (cut) k_synth<SOTS_SYNTH_4OP_SERIES, 1, false, 2, 3><<<grid, 4 * waves * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
#else
        if (cut && waves == 1) k_synth<SOTS_SYNTH_4OP_SERIES, 1, false, 2, 3><<<grid, 4 * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        else if (cut) k_synth<SOTS_SYNTH_4OP_SERIES, 2><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
#endif
        else k_synth<SOTS_SYNTH_4OP_SERIES, 0><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        break;
    case SOTS_SYNTH_TRIPLE_PAR:
        // up to 64 individuals per CU a wavefront per chain (three SIMDs): 134 -> ... us at P = 1024 (profiles/r03_experiments.md)
        if (allow_cut && waves == 1) k_synth<SOTS_SYNTH_TRIPLE_PAR, -1><<<grid, 3 * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        else k_synth<SOTS_SYNTH_TRIPLE_PAR, 0><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        break;
    default: return hipErrorInvalidValue;
    }
#undef SOTS_SYNTH_CASE
    return hipGetLastError();
}

hipError_t launch_window(hipStream_t st, float *audio, const float *window, uint32_t p, uint32_t log2n,
                         uint32_t pitch)
{
    const size_t total4 = ((size_t)p << log2n) / 4;
    k_window<<<grid_for(total4, 256, 8192), 256, 0, st>>>(audio, window, total4, log2n - 2, pitch / 4);
    return hipGetLastError();
}

// Grid of a grid-stride kernel whose items all cost the same: exactly as many workgroups as
// are resident at once (occupancy query, cached per kernel and per context: OccCache).  A larger grid runs in rounds
// and the last, partly filled round costs as much as a full one (measured: 4096 one-wave
// workgroups on 3072 slots took 1.5x the time of 3072).
template <typename K>
static uint32_t resident_grid(K kernel, int threads, uint32_t items, uint32_t num_cus, int *cache)
{
    if (*cache == 0) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess || per_cu < 1) per_cu = 1;
        *cache = per_cu;
    }
    const uint64_t cap = (uint64_t)(num_cus ? num_cus : 256) * (uint64_t)*cache;
    // (a grid balanced to equal row counts - 2979 workgroups of 22 rows instead of 3072 of 21 or 22 at P = 65536 - measures
    // the same: profiles/r03_experiments.md)
    return (uint32_t)(items < cap ? items : cap);
}

// The occupancy query of resident_grid and the launch: a call site names its instantiation once, as a function pointer
template <typename... KA, typename... A>
static hipError_t launch_resident(void (*kernel)(KA...), int threads, uint32_t items, uint32_t num_cus, int *cache, hipStream_t st, A... args)
{
    kernel<<<resident_grid(kernel, threads, items, num_cus, cache), threads, 0, st>>>(args...);
    return hipGetLastError();
}
constexpr uint32_t groups_of(uint32_t rows, uint32_t waves) { return (rows + waves - 1) / waves; } // workgroups of `waves` rows

// Which N has which kernel, each list written once (the lists decide what is instantiated): N <= 1024 runs on the
// wavefront-per-row kernels with LDS exchanges (k_fft, k_fitness), longer rows - and N = 256 (round 4): two complex points
// per lane, where k_fft's radix-4 / radix-8 passes need four or eight - on the wavefront-per-row kernels with the
// sub-transforms across lanes (k_fft_x, k_fitness_x; N = 1024 is instantiated for -DSOTS_X_MIN=10), N >= 16384 on the
// workgroup-per-row kernels (k_fft_big, k_fitness_big)
template <int... Ls> struct Log2nList {};
using WaveSizes = Log2nList<9, 10>;
using XSizes = Log2nList<8, 10, 11, 12, 13>;
using BigSizes = Log2nList<14, 15>;
// f(ic<L>{}) for the L of the list that equals log2n; `none` where the list has no such L.  (A left fold: f is instantiated
// in list order, and the order in which the launchers below first name the kernels is their order in the code object)
template <int... Ls, typename R, typename F>
static R for_log2n(Log2nList<Ls...>, uint32_t log2n, R none, F f)
{
    (void)(... || (log2n == (uint32_t)Ls && ((void)(none = f(ic<Ls>{})), true)));
    return none;
}
template <typename List> static bool has_log2n(List list, uint32_t log2n) { return for_log2n(list, log2n, false, [](auto) { return true; }); }

#ifndef SOTS_X_MIN
#define SOTS_X_MIN 11
#endif
static bool x_from(uint32_t log2n) { return has_log2n(XSizes{}, log2n) && (log2n == 8 || log2n >= SOTS_X_MIN); }
static bool big_from(uint32_t log2n) { return has_log2n(BigSizes{}, log2n); }

// N = 1024 from one row per resident wavefront (P >= 12 x CUs): one workgroup of twelve wavefronts per CU, rows dealt as
// the wavefronts ask (k_fft); 15.7 -> 14.7 us at P = 8192 already, level at 4096
static bool fft_wide(uint32_t p, uint32_t log2n, uint32_t num_cus)
{
#ifdef SOTS_FFT_NO_WIDE
    return false; // (experiments: the one-wavefront workgroups at every size)
#else
#ifndef SOTS_FFT_WIDE_ROWS
#define SOTS_FFT_WIDE_ROWS 1u
#endif
    return log2n == 10 && p >= SOTS_FFT_WIDE_ROWS * fft_wide_waves<10>() * (num_cus ? num_cus : 256u);
#endif
}

// The kernel choice of every spectral launcher, plain or segmented, staged or fused.  x_small: a small population, a
// wavefront per SIMD (k_fft_x with four wavefronts; the fused windowed form only, the others take it as x).  The threshold
// (fewer 16-row workgroups than CUs) was measured at N = 4096 and 2048, where x_waves is 16; N = 8192 (x_waves 8) follows
// it unmeasured
enum class Spectral { none, wave, wide, x, x_small, big };
static Spectral spectral_choice(uint32_t p, uint32_t log2n, uint32_t num_cus)
{
    if (big_from(log2n)) return Spectral::big;
    if (x_from(log2n)) return groups_of(p, x_waves<12>()) < (num_cus ? num_cus : 256u) ? Spectral::x_small : Spectral::x;
    if (fft_wide(p, log2n, num_cus)) return Spectral::wide;
    return has_log2n(WaveSizes{}, log2n) ? Spectral::wave : Spectral::none;
}

// The lookup of every launch that files keys (kernels/sel_keys.h), the spectral kernel's and the staged k_bucket_fitness's
// alike, so that a staged and a fused run of one population file by the same code: two levels up to 65 536 rows, where they
// won every round (1.4-1.5 us of 113-115 per generation, profiles/r30_experiments.md), all bounds against every key above,
// where the two levels lost 4.4 us of 212 at 131 072 rows (profiles/r19_experiments.md).  The buckets are the same either way.
#ifndef SOTS_BKT_TWO_LEVEL_MAX_P
#define SOTS_BKT_TWO_LEVEL_MAX_P 65536u // (0u: the build variant that files flat at every size)
#endif
static bool bkt_two_level(uint32_t p) { return p <= SOTS_BKT_TWO_LEVEL_MAX_P; }

// a workgroup per row: as many workgroups as rows, at most four per CU (they loop)
static uint32_t big_grid(uint32_t p, uint32_t num_cus)
{
    const uint32_t cap = 4u * (num_cus ? num_cus : 256u);
    return p < cap ? p : cap;
}
template <int L, int MODE, bool WIN, bool SEG = false, int OBJ = kObjMagnitude, bool WGT = false, typename... FL>
static hipError_t launch_fft_big(hipStream_t st, uint32_t p, uint32_t num_cus, const float *audio, float *spectrum, const float *target,
                                 float *fitness, const float2 *tw, const float *window, float inv_n, float inv_wf, uint32_t pitch, FL... fl)
{
    const auto kernel = k_fft_big<L, MODE, WIN, SEG, OBJ, WGT, FL...>;
    const size_t lds = ((size_t)(1u << L) / 2u) * sizeof(float2) + 64u;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    kernel<<<big_grid(p, num_cus), kBigThreads, lds, st>>>(audio, spectrum, target, fitness, tw, window, p, inv_n, inv_wf, pitch, fl...);
    return hipGetLastError();
}

hipError_t launch_fft(hipStream_t st, const float *audio, float *spectrum, const float2 *twiddle,
                      uint32_t p, uint32_t log2n, uint32_t pitch, uint32_t num_cus, OccCache *oc)
{
    constexpr int W = fft_wide_waves<10>();
    switch (spectral_choice(p, log2n, num_cus)) {
    case Spectral::big:
        return for_log2n(BigSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
            return launch_fft_big<decltype(l)::value, 0, false>(st, p, num_cus, audio, spectrum, nullptr, nullptr, twiddle, nullptr, 0.f, 0.f, pitch);
        });
    case Spectral::wide:
        return launch_resident(k_fft<10, 0, false, W>, W * kWave, groups_of(p, W), num_cus, &oc->wide[0], st, audio, spectrum, nullptr, nullptr, twiddle, nullptr, p, 0.f, 0.f, pitch);
    case Spectral::x_small: // (no four-wavefront form)
    case Spectral::x:
        return for_log2n(XSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
            constexpr int L = decltype(l)::value, WG = x_waves<L, 0>();
            return launch_resident(k_fft_x<L, 0, false>, WG * kWave, groups_of(p, WG), num_cus, &oc->x_fft[L], st, audio, spectrum, nullptr, nullptr, twiddle, nullptr, p, 0.f, 0.f, pitch, nullptr);
        });
    case Spectral::wave:
        return for_log2n(WaveSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
            constexpr int L = decltype(l)::value;
            return launch_resident(k_fft<L, 0, false>, kWave, p, num_cus, &oc->fft[L], st, audio, spectrum, nullptr, nullptr, twiddle, nullptr, p, 0.f, 0.f, pitch);
        });
    default: return hipErrorInvalidValue;
    }
}

// The objective and the weights of a launch as template arguments: f(ic<OBJ>{}, bool_constant<WGT>{}, fl...), where fl holds
// the log objective's floor and then the weighted kernels' table u (the kernels' last arguments); the unweighted magnitude
// instantiations are launched exactly as before there was a choice
template <typename F>
static hipError_t with_objective(const Objective &obj, const float *u, F f)
{
    if (obj.kind == SOTS_OBJECTIVE_LOG_MAGNITUDE) {
        if (u) return f(ic<kObjLogMagnitude>{}, std::true_type{}, obj.floor, u);
        return f(ic<kObjLogMagnitude>{}, std::false_type{}, obj.floor);
    }
    if (obj.kind != SOTS_OBJECTIVE_MAGNITUDE) return hipErrorInvalidValue;
    if (u) return f(ic<kObjMagnitude>{}, std::true_type{}, u);
    return f(ic<kObjMagnitude>{}, std::false_type{});
}

hipError_t launch_fitness(hipStream_t st, const float *spectrum, const float *target, float *fitness,
                          uint32_t p, uint32_t log2n, float inv_n, float inv_wf, uint32_t num_cus, OccCache *oc, const Objective &obj)
{
    // (the staged kernels index the plain weight table by bin)
    return with_objective(obj, obj.weights, [&](auto o, auto w, auto... fl) {
        constexpr int OBJ = decltype(o)::value;
        constexpr bool WGT = decltype(w)::value;
        switch (spectral_choice(p, log2n, num_cus)) {
        case Spectral::big:
            return for_log2n(BigSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
                k_fitness_big<decltype(l)::value, OBJ, WGT, decltype(fl)...><<<big_grid(p, num_cus), kBigThreads, 0, st>>>(spectrum, target, fitness, p, inv_n, inv_wf, fl...);
                return hipGetLastError();
            });
        case Spectral::x_small: // (no four-wavefront form)
        case Spectral::x:
            return for_log2n(XSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
                constexpr int L = decltype(l)::value, WG = x_waves<L>();
                return launch_resident(k_fitness_x<L, OBJ, WGT, decltype(fl)...>, WG * kWave, groups_of(p, WG), num_cus, &oc->x_fitness[L], st, spectrum, target, fitness, p, inv_n, inv_wf, fl...);
            });
        case Spectral::wide: // (a wavefront per workgroup at every population)
        case Spectral::wave:
            return for_log2n(WaveSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
                constexpr int L = decltype(l)::value;
                return launch_resident(k_fitness<L, OBJ, WGT, decltype(fl)...>, kWave, p, num_cus, &oc->fitness[L], st, spectrum, target, fitness, p, inv_n, inv_wf, fl...);
            });
        default: return hipErrorInvalidValue;
        }
    });
}

hipError_t launch_objective_map(hipStream_t st, float *dst, const float *src, size_t n, float floor)
{
    if (n == 0) return hipSuccess;
    k_objective_map<<<grid_for(n, 256, 8192), 256, 0, st>>>(dst, src, n, floor);
    return hipGetLastError();
}

// the table image the fused long-row kernel copies in (bytes: x_table_bytes; rebuilt whenever the target changes)
size_t x_table_bytes(uint32_t log2n)
{
    return for_log2n(XSizes{}, log2n, (size_t)0, [](auto l) {
        constexpr int L = decltype(l)::value;
        return x_applies<L>() ? x_table_floats<L>() * sizeof(float) : (size_t)0; // (N = 256 makes its tables in the workgroup)
    });
}
hipError_t launch_x_tables(hipStream_t st, float *image, const float2 *twiddle, const float *window, const float *target, uint32_t log2n)
{
    if (!x_from(log2n)) return hipSuccess;
    hipError_t e = hipMemsetAsync(image, 0, x_table_bytes(log2n), st); // (the padding between the lanes' rows)
    if (e != hipSuccess) return e;
    return for_log2n(XSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
        k_x_tables<decltype(l)::value><<<8, 256, 0, st>>>(image, twiddle, window, target);
        return hipGetLastError();
    });
}

// The fused launch, plain (SEG = false: `target` is the one target, or the table image of k_fft_x) or segmented (every row
// against its chunk's target in the image `target`): one routine, so the same kernel choice for the same row count, and the
// same OccCache slots.  The forms without a window exist for the plain unweighted magnitude objective only (RAW; the library
// itself always passes its window; the log N = 4096 form without one would not fit its 128 registers): elsewhere a missing
// window is an error, not another kernel.  `lists`: the bucketing instantiation (plain only), or nothing - a caller that
// counts on the lists must not get a launch without them
template <bool SEG, int OBJ, bool WGT, typename... FL>
static hipError_t launch_fused(hipStream_t st, const float *audio, const float *window, const float *target, float *fitness,
                               const float2 *twiddle, uint32_t p, uint32_t log2n, uint32_t pitch, float inv_n, float inv_wf,
                               uint32_t num_cus, OccCache *oc, const SelLists *lists, FL... fl)
{
    constexpr bool RAW = !SEG && OBJ == kObjMagnitude && !WGT;
    constexpr int W = fft_wide_waves<10>();
    if (!RAW && !window) return hipErrorInvalidValue;
    if (lists) {
        if constexpr (SEG) return hipErrorInvalidValue;
        else {
            if (!window || !select_lists_apply(p, log2n, num_cus) || lists->buckets != select_splitter_count(num_cus) || !lists->slot || !lists->cnt || !lists->lists)
                return hipErrorInvalidValue;
            const auto file = [&](auto l) { // (l: the lists, typed by the lookup)
                return launch_resident(k_fft<10, 1, true, W, false, true, OBJ, WGT, decltype(l), FL...>, W * kWave, groups_of(p, W), num_cus, &oc->wide[3], st,
                                       audio, nullptr, target, fitness, twiddle, window, p, inv_n, inv_wf, pitch, l, fl...);
            };
            return bkt_two_level(p) ? file(SelListsTwoLevel{*lists}) : file(*lists);
        }
    }
    // f(bool_constant<WIN>{}): with the window, or without one where that form exists
    const auto with_window = [&](auto f) {
        if (window) return f(std::true_type{});
        if constexpr (RAW) return f(std::false_type{});
        return hipErrorInvalidValue;
    };
    const Spectral choice = spectral_choice(p, log2n, num_cus);
    switch (choice) {
    case Spectral::big: // (size outside, window inside: the order of these kernels in the code object)
        return for_log2n(BigSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
            return with_window([&](auto win) {
                return launch_fft_big<decltype(l)::value, 1, decltype(win)::value, SEG, OBJ, WGT, FL...>(st, p, num_cus, audio, nullptr, target, fitness, twiddle, window, inv_n, inv_wf, pitch, fl...);
            });
        });
    case Spectral::x_small:
    case Spectral::x:
        return with_window([&](auto win) {
            constexpr bool WIN = decltype(win)::value;
            if constexpr (WIN) { // (no four-wavefront form without a window)
                if (choice == Spectral::x_small)
                    return for_log2n(XSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
                        constexpr int L = decltype(l)::value;
                        return launch_resident(k_fft_x<L, 1, true, 4, SEG, OBJ, WGT, FL...>, 4 * kWave, groups_of(p, 4), num_cus, &oc->x_small[L], st,
                                               audio, nullptr, target, fitness, twiddle, window, p, inv_n, inv_wf, pitch, oc->x_image, fl...);
                    });
            }
            return for_log2n(XSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
                constexpr int L = decltype(l)::value, WG = x_waves<L>();
                return launch_resident(k_fft_x<L, 1, WIN, WG, SEG, OBJ, WGT, FL...>, WG * kWave, groups_of(p, WG), num_cus, WIN ? &oc->x_fused_win[L] : &oc->x_fused_raw[L], st,
                                       audio, nullptr, target, fitness, twiddle, window, p, inv_n, inv_wf, pitch, WIN ? oc->x_image : nullptr, fl...);
            });
        });
    case Spectral::wide:
        return with_window([&](auto win) {
            constexpr bool WIN = decltype(win)::value;
            return launch_resident(k_fft<10, 1, WIN, W, SEG, false, OBJ, WGT, FL...>, W * kWave, groups_of(p, W), num_cus, &oc->wide[WIN ? 1 : 2], st,
                                   audio, nullptr, target, fitness, twiddle, window, p, inv_n, inv_wf, pitch, fl...);
        });
    case Spectral::wave:
        return with_window([&](auto win) {
            constexpr bool WIN = decltype(win)::value;
            return for_log2n(WaveSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
                constexpr int L = decltype(l)::value;
                return launch_resident(k_fft<L, 1, WIN, 1, SEG, false, OBJ, WGT, FL...>, kWave, p, num_cus, WIN ? &oc->fused_win[L] : &oc->fused_raw[L], st,
                                       audio, nullptr, target, fitness, twiddle, window, p, inv_n, inv_wf, pitch, fl...);
            });
        });
    default: return hipErrorInvalidValue;
    }
}

// obj.weights_image holds u in the layout of the kernel's target table (one table for all chunks of a segmented launch)
template <bool SEG>
static hipError_t launch_fused_objective(hipStream_t st, const float *audio, const float *window, const float *target, float *fitness,
                                         const float2 *twiddle, uint32_t p, uint32_t log2n, uint32_t pitch, float inv_n, float inv_wf,
                                         uint32_t num_cus, OccCache *oc, const SelLists *lists, const Objective &obj)
{
    if (obj.weights && !obj.weights_image) return hipErrorInvalidValue;
    return with_objective(obj, obj.weights ? weight_table(obj.weights_image) : nullptr, [&](auto o, auto w, auto... fl) {
        return launch_fused<SEG, decltype(o)::value, decltype(w)::value>(st, audio, window, target, fitness, twiddle, p, log2n, pitch, inv_n, inv_wf, num_cus, oc, lists, fl...);
    });
}

hipError_t launch_fft_fitness(hipStream_t st, const float *audio, const float *window, const float *target,
                              float *fitness, const float2 *twiddle, uint32_t p, uint32_t log2n, uint32_t pitch,
                              float inv_n, float inv_wf, uint32_t num_cus, OccCache *oc, const SelLists *lists, const Objective &obj)
{
    return launch_fused_objective<false>(st, audio, window, target, fitness, twiddle, p, log2n, pitch, inv_n, inv_wf, num_cus, oc, lists, obj);
}

constexpr uint32_t kSortMaxTiles = 256;
constexpr uint32_t kSortTwoLevelFrom = 131072; // padded population from which runs of 8 tiles are merged first

// Plans: one LDS tile (n_pad <= 4096); tiles of 1024 + one rank level (up to 65536: 64 tiles);
// tiles of 1024 merged into runs of 8192 + a rank level over the runs (two levels: the rank work is
// quadratic in the number of sorted pieces, 128 tiles -> 16 runs at 131072); beyond 128 runs
// (n_pad > 1M) global bitonic steps over tiles of 4096.
constexpr uint32_t kSortMaxRuns = 128;         // 1 Mi keys; the counts of the run level take runs * n_pad * 2 bytes
static bool sort_two_level(uint32_t n_pad) { return n_pad >= kSortTwoLevelFrom && n_pad / kRankLdsKeys <= kSortMaxRuns; }

static void sort_plan(uint32_t n_pad, uint32_t &tile, uint32_t &tiles)
{
    if (n_pad <= kSortSmall) tile = n_pad; // (k_sort_small: no tiles at all)
    else if (n_pad <= 65536u || sort_two_level(n_pad)) tile = 1024u;
    else tile = kSortTile;
    tiles = n_pad / tile;
}

// tiles staged per rank workgroup: as many as fit the LDS buffer and a 16-bit count
static uint32_t rank_group(uint32_t tile, uint32_t tiles)
{
    uint32_t group = kRankLdsKeys / tile;
    if (group > kRankGroup) group = kRankGroup;
    if (group < 1) group = 1;
    while (group > tiles) group >>= 1;
    return group;
}

// scratch layout: [partial counts (u16)] then, for two levels, [merged runs (u64, n_pad keys)]
static size_t sort_partial_bytes(uint32_t n_pad)
{
    uint32_t tile, tiles;
    sort_plan(n_pad, tile, tiles);
    if (sort_two_level(n_pad)) return (size_t)(n_pad / kRankLdsKeys) * n_pad * sizeof(uint16_t);
    if (tiles <= 1 || tiles > kSortMaxTiles) return 16;
    const uint32_t group = rank_group(tile, tiles);
    return (size_t)(tiles / group) * n_pad * sizeof(uint16_t);
}

size_t sort_scratch_bytes(uint32_t p)
{
    const uint32_t n_pad = next_pow2(p < 2 ? 2 : p);
    size_t bytes = (sort_partial_bytes(n_pad) + 255) & ~(size_t)255;
    if (sort_two_level(n_pad)) bytes += (size_t)n_pad * sizeof(uint64_t);
    return bytes;
}

hipError_t launch_sort(hipStream_t st, const float *vin, const float *sin, const float *fin,
                       float *vout, float *sout, float *fout, uint64_t *keys, void *scratch, uint32_t p,
                       uint32_t d, uint32_t first_row, const SortExchange *exchange)
{
    const SortExchange ex = exchange ? *exchange : SortExchange{};
    const uint32_t n_pad = next_pow2(p < 2 ? 2 : p);
    if (n_pad <= kSortSmall) { // one launch
        switch ((n_pad + kWave - 1) / kWave) {
        case 1: k_sort_small<1><<<1, 1 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, first_row, ex); break;
        case 2: k_sort_small<2><<<1, 2 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, first_row, ex); break;
        case 4: k_sort_small<4><<<1, 4 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, first_row, ex); break;
        case 8: k_sort_small<8><<<1, 8 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, first_row, ex); break;
        default: k_sort_small<16><<<1, 16 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, first_row, ex); break;
        }
        return hipGetLastError();
    }
    uint32_t tile, tiles;
    sort_plan(n_pad, tile, tiles);
    uint32_t threads = tile / 2;
    threads = threads < 64 ? 64 : threads > (uint32_t)kSortThreads ? (uint32_t)kSortThreads : threads;
    const bool two_level = sort_two_level(n_pad);
    const bool rank_merge = two_level || (tiles > 1 && tiles <= kSortMaxTiles);
    if (rank_merge && tile == 4 * kRunKeys)
        k_sort_tiles_1k<<<tiles, 256, 0, st>>>(fin, keys, p);
    else
        k_sort_tiles<<<tiles, threads, 0, st>>>(fin, keys, p, tile, rank_merge ? 0u : 1u);
    if (two_level) {
        uint16_t *partial = static_cast<uint16_t *>(scratch);
        uint64_t *merged = reinterpret_cast<uint64_t *>(static_cast<char *>(scratch) +
                                                        ((sort_partial_bytes(n_pad) + 255) & ~(size_t)255));
        // level 1: groups of 8 tiles -> sorted runs of 8192 keys; level 2: every key against every run
        k_sort_rank_pairs<kRankGroup, true><<<tiles, kRankThreads, 0, st>>>(keys, nullptr, n_pad, tile, merged);
        const uint32_t runs = n_pad / kRankLdsKeys;
        k_sort_rank_pairs<1><<<dim3(runs, runs), kRankThreads, 0, st>>>(merged, partial, n_pad, kRankLdsKeys);
        k_sort_rank_scatter<<<n_pad / 64, kRankThreads, 0, st>>>(merged, partial, vin, sin, fin, vout, sout, fout,
                                                               n_pad, runs, p, d, first_row, ex);
        return hipGetLastError();
    }
    if (rank_merge) {
        uint16_t *partial = static_cast<uint16_t *>(scratch);
        const uint32_t group = rank_group(tile, tiles), groups = tiles / group;
        switch (group) {
        case 8: k_sort_rank_pairs<8><<<dim3(tiles, groups), kRankThreads, 0, st>>>(keys, partial, n_pad, tile); break;
        case 4: k_sort_rank_pairs<4><<<dim3(tiles, groups), kRankThreads, 0, st>>>(keys, partial, n_pad, tile); break;
        case 2: k_sort_rank_pairs<2><<<dim3(tiles, groups), kRankThreads, 0, st>>>(keys, partial, n_pad, tile); break;
        default: k_sort_rank_pairs<1><<<dim3(tiles, groups), kRankThreads, 0, st>>>(keys, partial, n_pad, tile); break;
        }
        k_sort_rank_scatter<<<n_pad / 64, kRankThreads, 0, st>>>(keys, partial, vin, sin, fin, vout, sout, fout,
                                                               n_pad, groups, p, d, first_row, ex);
        return hipGetLastError();
    }
    for (uint32_t k = tile << 1; k <= n_pad && k != 0; k <<= 1) {
        for (uint32_t j = k >> 1; j >= tile; j >>= 1)
            k_sort_global_step<<<grid_for(n_pad / 2, 256), 256, 0, st>>>(keys, n_pad, k, j);
        k_sort_tile_merge<<<tiles, threads, 0, st>>>(keys, k, tile);
    }
    k_sort_gather<<<grid_for((uint64_t)p * (2 * d + 1), 256), 256, 0, st>>>(keys, vin, sin, fin, vout, sout,
                                                                            fout, p, d, first_row, ex);
    return hipGetLastError();
}

// keys buffer: n_pad 64-bit keys (full sort) or n_pad fitness-bit words + n_pad indices (selection),
// followed by the selection's per-tile samples
// The selection's key arrays: the population padded to a power of two and to at least kSelMinTiles tiles (the rank kernel
// holds one sample per lane and more: 16 tiles x 4 samples); a population of 2048 ... 8192 simply has tiles of nothing but
// padding keys behind its own (they sort last, stage one quantum each and move nothing)
static uint32_t sel_pad(uint32_t p)
{
    const uint32_t n_pad = next_pow2(p < 2 ? 2 : p);
    return n_pad < kSelMinTiles * kSelTile ? kSelMinTiles * kSelTile : n_pad;
}

size_t sort_keys_bytes(uint32_t p)
{
    const uint32_t n_pad = p > kSortSmall ? sel_pad(p) : next_pow2(p < 2 ? 2 : p);
    return (size_t)n_pad * sizeof(uint64_t) + (size_t)2 * kSelMaxTiles * kSelSamples * sizeof(uint32_t);
}

// The selection applies to every population that does not fit k_sort_small's one launch (P > 1024; round 3: it used to start at
// 8192, the three launches of the tile sort below that took 20-23 us where the selection's two take 15) while at most half of
// the rows are wanted (beyond that nearly everything would be staged and the full sort is the better plan).  Up to 64 tiles
// (P <= 65536) the rank kernel works on the 1024-key tiles; at 128 tiles (P <= 131072) they are first merged four by four
// (k_sel_merge4), which quarters its work; larger populations take the two-level full sort.
constexpr uint32_t kSelDirectTiles = 64, kSelMergedTiles = 128;
bool select_applies(uint32_t p, uint32_t need)
{
    const uint32_t tiles = sel_pad(p) / kSelTile;
    return p > kSortSmall && tiles <= kSelMergedTiles && need >= 1 && (uint64_t)need * 2 <= p;
}

// scratch of the merged plan: the 4096-key tiles (bits, indices) and their samples
size_t select_scratch_bytes(uint32_t p)
{
    const uint32_t n_pad = sel_pad(p);
    return (size_t)n_pad * 2 * sizeof(uint32_t) + (size_t)2 * kSelMaxTiles * kSelSamples * sizeof(uint32_t);
}

hipError_t launch_select(hipStream_t st, const float *vin, const float *sin, const float *fin, float *vout,
                         float *sout, float *fout, uint64_t *keys, void *scratch, uint32_t p, uint32_t d, uint32_t need,
                         uint32_t num_cus, const SortExchange *exchange)
{
    if (!select_applies(p, need)) return hipErrorInvalidValue;
    const SortExchange ex = exchange ? *exchange : SortExchange{};
    const uint32_t n_pad = sel_pad(p);
    const uint32_t tiles = n_pad / kSelTile;
    uint32_t *kbits = reinterpret_cast<uint32_t *>(keys), *kidx = kbits + n_pad, *samples = kidx + n_pad;
    // (split while the parts still find CUs of their own; the 128 tiles of P = 131072 stay whole)
    if (SOTS_SEL_SPLIT > 1 && tiles * SOTS_SEL_SPLIT <= (num_cus ? num_cus : 256))
        k_sel_tiles<SOTS_SEL_SPLIT><<<tiles * SOTS_SEL_SPLIT, kSelTile, 0, st>>>(fin, kbits, kidx, samples, p, tiles);
    else k_sel_tiles<1><<<tiles, kSelTile, 0, st>>>(fin, kbits, kidx, samples, p, tiles);
    // one workgroup per CU (the staging buffer takes the LDS); more only when a share of the staged
    // positions would exceed the per-workgroup key store
    uint32_t grid = num_cus ? num_cus : 256;
    const uint32_t min_grid = (tiles * kSelTile + kSelMaxOwn - 1) / kSelMaxOwn;
    if (grid < min_grid) grid = min_grid;
    // lanes per key x 8 search chains = the tiles one pass stages: 64 / 32 / 16 tiles of 1024 keys, <= 20 big tiles
    // at most 8 real tiles (P <= 8192): they are staged whole (32 KiB), the padding tiles not at all
    const uint32_t real_tiles = (p + kSelTile - 1) / kSelTile, whole = real_tiles <= 8 ? real_tiles : 0u;
#define SOTS_SEL(R, T, Q, L, KB, KI, SM, NT) \
    k_sel_rank_scatter<R, T, Q, L><<<grid, kSelThreads, 0, st>>>(KB, KI, SM, vin, sin, fin, vout, sout, fout, NT, need, p, d, ex, whole)
    if (tiles <= kSelDirectTiles) {
        switch (tiles * kSelSamples / kWave) {
        case 1: SOTS_SEL(1, kSelTile, kSelQuantum, 2, kbits, kidx, samples, tiles); break;
        case 2: SOTS_SEL(2, kSelTile, kSelQuantum, 4, kbits, kidx, samples, tiles); break;
        case 4: SOTS_SEL(4, kSelTile, kSelQuantum, 8, kbits, kidx, samples, tiles); break;
        default: return hipErrorInvalidValue;
        }
    } else {
        uint32_t *bbits = static_cast<uint32_t *>(scratch), *bidx = bbits + n_pad, *bsamples = bidx + n_pad;
        const uint32_t big = tiles / 4;
        k_sel_merge4<<<big, kSelTile, 0, st>>>(kbits, kidx, bbits, bidx, bsamples);
        switch (big * kSelBigSamples / kWave) {
        case 4: SOTS_SEL(4, kSelBigTile, kSelBigQuantum, 4, bbits, bidx, bsamples, big); break;
        default: return hipErrorInvalidValue;
        }
    }
#undef SOTS_SEL
    return hipGetLastError();
}

// ---- the one-launch selection between stored splitters (k_sel_splitters) ----
// a slot: one splitter per workgroup, one workgroup per CU
uint32_t select_splitter_count(uint32_t num_cus)
{
    const uint32_t b = num_cus ? num_cus : 256;
    return b > kSplMaxBuckets ? kSplMaxBuckets : b < 2 ? 2 : b;
}
size_t select_splitter_slot_bytes() { return (size_t)kSplMaxBuckets * sizeof(uint64_t); }
// positions q * step of one generation's order are the next one's splitters: the old order up to 1.25 * need.  While a
// run improves, the next generation puts 1.3 ... 4 times as many keys below an old key as the old generation did
// (profiles/r06_experiments.md); a converged population whose fitness values all tie puts exactly as many.  The cut
// of the next generation must fall inside the slot: behind the last splitter one workgroup owns all the rest.
static uint32_t select_splitter_step(uint32_t need, uint32_t buckets)
{
    return (uint32_t)(((uint64_t)need * 5 / 4 + buckets - 2) / (buckets - 1)); // >= 1 (need >= 1); (buckets - 1) * step < P as need <= P / 2
}

hipError_t launch_select_splitters(hipStream_t st, const float *vin, const float *sin, const float *fin, float *vout,
                                   float *sout, float *fout, uint64_t *keys, const uint64_t *spl_in, uint64_t *spl_out,
                                   uint32_t p, uint32_t d, uint32_t need, uint32_t num_cus, const SortExchange *exchange,
                                   const SelLists *lists)
{
    if (!select_applies(p, need)) return hipErrorInvalidValue;
    const SortExchange ex = exchange ? *exchange : SortExchange{};
    const uint32_t buckets = select_splitter_count(num_cus);
    if (lists && (buckets > kSelListMaxBuckets || lists->buckets != buckets || lists->slot != spl_in || !lists->cnt || !lists->cnt_other || !lists->lists)) return hipErrorInvalidValue;
    // bit 0: the fitness can be read 16 bytes per lane; bit 1: so can rows of four genes
    const uintptr_t row_bits = reinterpret_cast<uintptr_t>(vin) | reinterpret_cast<uintptr_t>(sin) | reinterpret_cast<uintptr_t>(vout) | reinterpret_cast<uintptr_t>(sout);
    const uint32_t vec = ((reinterpret_cast<uintptr_t>(fin) & 15u) == 0 ? 1u : 0u) | ((row_bits & 15u) == 0 ? 2u : 0u);
    k_sel_splitters<<<buckets, kSplThreads, 0, st>>>(vin, sin, fin, vout, sout, fout, spl_in, spl_out, keys, p, need,
                                                     select_splitter_step(need, buckets), d, ex, vec, lists ? *lists : SelLists{});
    return hipGetLastError();
}

// ---- list mode: who files the keys ----
bool select_lists_apply(uint32_t p, uint32_t log2n, uint32_t num_cus)
{
    return fft_wide(p, log2n, num_cus) && select_splitter_count(num_cus) <= kBktMaxBuckets;
}
size_t select_lists_bytes(uint32_t num_cus) { return (size_t)select_splitter_count(num_cus) * kSelListCap * sizeof(uint64_t); }
size_t select_counters_bytes() { return (size_t)kSelListMaxBuckets * kSelListShards * sizeof(uint32_t); }

// bkt_visit over an array of fitness values: a wavefront takes 64 consecutive keys, one after the other (the visit is
// a wavefront's, its key uniform)
constexpr uint32_t kBktThreads = 256;
template <int LK>
static __global__ __launch_bounds__(kBktThreads) void k_bucket_fitness(const float *__restrict__ fin, uint32_t p_len, SelLists bk)
{
    __shared__ __attribute__((aligned(8))) uint32_t bnd_s[2 * kBktMaxBuckets];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    if (tid < kWave) bkt_bounds<LK>(bk.slot, bk.buckets, bnd_s, lane);
    __syncthreads();
    const uint64_t last = bkt_last<LK>(bnd_s, bk.buckets);
    const uint32_t first = __builtin_amdgcn_readfirstlane(blockIdx.x * kBktThreads + (tid & ~(kWave - 1)));
    const uint32_t idx = first + lane;
    const uint32_t bits = idx < p_len ? order_bits(fin[idx]) : 0u;
    BktPend pd = {0ull, kBktNone, 0u};
    for (uint32_t l = 0; l < kWave && first + l < p_len; ++l) {
        const uint32_t kb = (uint32_t)__builtin_amdgcn_readlane((int)bits, (int)l);
        bkt_visit<LK>(bk, bnd_s, last, ((uint64_t)kb << 32) | (first + l), (first / kWave) % kSelListShards, lane, pd);
    }
    bkt_flush(bk, pd, lane);
}

hipError_t launch_bucket_fitness(hipStream_t st, const float *fitness, uint32_t p, const SelLists &lists)
{
    if (lists.buckets < 2 || lists.buckets > kBktMaxBuckets || !lists.slot || !lists.cnt || !lists.lists) return hipErrorInvalidValue;
    const uint32_t grid = (p + kBktThreads - 1) / kBktThreads;
    if (bkt_two_level(p)) k_bucket_fitness<kBktTwoLevel><<<grid, kBktThreads, 0, st>>>(fitness, p, lists);
    else k_bucket_fitness<kBktFlat><<<grid, kBktThreads, 0, st>>>(fitness, p, lists);
    return hipGetLastError();
}

hipError_t launch_select_seed(hipStream_t st, const float *fsorted, uint64_t *spl_out, uint32_t need, uint32_t num_cus)
{
    const uint32_t buckets = select_splitter_count(num_cus);
    k_sel_seed<<<1, kSplMaxBuckets, 0, st>>>(fsorted, spl_out, need, select_splitter_step(need, buckets), buckets);
    return hipGetLastError();
}

hipError_t launch_pack_rows(hipStream_t st, const float *values, const float *steps, const float *fitness,
                            float *rows, uint32_t first_row, uint32_t n_rows, uint32_t d)
{
    if (n_rows == 0) return hipSuccess;
    k_pack_rows<<<grid_for((uint64_t)n_rows * (2 * d + 1), 256), 256, 0, st>>>(values, steps, fitness, rows,
                                                                               first_row, n_rows, d);
    return hipGetLastError();
}

hipError_t launch_unpack_rows(hipStream_t st, float *values, float *steps, float *fitness,
                              const float *rows, uint32_t first_row, uint32_t n_rows, uint32_t d,
                              uint32_t skip_first, uint32_t skip_count)
{
    if (n_rows == 0) return hipSuccess;
    k_unpack_rows<<<grid_for((uint64_t)n_rows * (2 * d + 1), 256), 256, 0, st>>>(values, steps, fitness, rows,
                                                                                 first_row, n_rows, d, skip_first,
                                                                                 skip_count);
    return hipGetLastError();
}

// ---- chunks in flight ----------------------------------------------------------------
hipError_t launch_init_population_seg(hipStream_t st, float *values, float *steps, float *fitness, const PopDims &pd,
                                      uint32_t first_chunk, uint32_t chunks)
{
    k_init_population_seg<<<grid_for((uint64_t)chunks * pd.p * pd.d, 256), 256, 0, st>>>(values, steps, fitness, pd, first_chunk, chunks);
    return hipGetLastError();
}

hipError_t launch_recombine_mutate_seg(hipStream_t st, const float *vin, const float *sin, float *vout, float *sout,
                                       const PopDims &pd, const MutateConsts &mc, uint32_t generation, uint32_t chunks)
{
    k_recombine_mutate_seg<<<grid_for((uint64_t)chunks * pd.p * pd.d, 256), 256, 0, st>>>(vin, sin, vout, sout, pd, mc, generation, chunks);
    return hipGetLastError();
}

size_t seg_target_stride(uint32_t log2n)
{
    const size_t bins = (1u << log2n) / 2u;
    if (!x_from(log2n)) return bins;
    return for_log2n(XSizes{}, log2n, bins, [](auto l) { return (size_t)x_seg_stride<decltype(l)::value>(); });
}

size_t seg_target_bytes(uint32_t log2n, uint32_t chunks)
{
    return (kSegHead + (size_t)chunks * seg_target_stride(log2n)) * sizeof(float);
}

hipError_t launch_seg_targets(hipStream_t st, float *image, const float *targets, uint32_t log2n, uint32_t chunks)
{
    float *tables = image + kSegHead;
    if (!x_from(log2n))
        return hipMemcpyAsync(tables, targets, (size_t)chunks * ((1u << log2n) / 2u) * sizeof(float), hipMemcpyDeviceToDevice, st);
    const uint64_t work = (uint64_t)chunks * (1u << log2n) / 2u;
    return for_log2n(XSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
        k_x_seg_targets<decltype(l)::value><<<grid_for(work, 256), 256, 0, st>>>(tables, targets, chunks);
        return hipGetLastError();
    });
}

// The weight table of the fused kernels: u[N/2] laid out as ONE chunk's target table (plain bins for k_fft and k_fft_big,
// the per-(lane, register) table for k_fft_x), so the weighted kernels read u wherever they read the target
size_t weight_image_bytes(uint32_t log2n) { return seg_target_bytes(log2n, 1); }
hipError_t launch_weight_image(hipStream_t st, float *image, const float *u, uint32_t log2n)
{
    const hipError_t e = hipMemsetAsync(image, 0, weight_image_bytes(log2n), st); // (the padding entries are never read; they are defined all the same)
    if (e != hipSuccess) return e;
    return launch_seg_targets(st, image, u, log2n, 1);
}

// launch_fft_fitness with a window, every row against its chunk's target: each kernel's SEG instantiation
hipError_t launch_fft_fitness_seg(hipStream_t st, const float *audio, const float *window, const float *seg_image, float *fitness,
                                  const float2 *twiddle, uint32_t p, uint32_t log2n, uint32_t pitch, float inv_n, float inv_wf,
                                  uint32_t num_cus, OccCache *oc, const Objective &obj)
{
    return launch_fused_objective<true>(st, audio, window, seg_image, fitness, twiddle, p, log2n, pitch, inv_n, inv_wf, num_cus, oc, nullptr, obj);
}

hipError_t launch_sort_seg(hipStream_t st, const float *vin, const float *sin, const float *fin, float *vout, float *sout,
                           float *fout, uint32_t p, uint32_t d, uint32_t chunks)
{
    const uint32_t n_pad = next_pow2(p < 2 ? 2 : p);
    if (n_pad > kSortSmall) return hipErrorInvalidValue;
    const SortExchange ex{};
    switch ((n_pad + kWave - 1) / kWave) {
    case 1: k_sort_small<1, true><<<chunks, 1 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, 0, ex); break;
    case 2: k_sort_small<2, true><<<chunks, 2 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, 0, ex); break;
    case 4: k_sort_small<4, true><<<chunks, 4 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, 0, ex); break;
    case 8: k_sort_small<8, true><<<chunks, 8 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, 0, ex); break;
    default: k_sort_small<16, true><<<chunks, 16 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, 0, ex); break;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// run record (sots_track): best-ever individual and per-generation history, one workgroup per chunk, right after a
// generation's sortPopulation.  Reads rows 0..numParents-1 of the sorted half only - every sort mode and both selection
// plans place those each generation - and writes nothing the generation loop reads.
// ------------------------------------------------------------------------------------
namespace {

// A context's 16384 parents are a quarter of a million floats for ONE workgroup: 1024 threads with sixteen loads in flight
// each keep that to a few memory round trips; a few dozen parents (chunks in flight) take four wavefronts.  The choice
// is a function of the row count and D alone, like everything else that shapes the sums.
constexpr uint32_t kTrackThreadsSmall = 256, kTrackThreadsLarge = 1024;
constexpr uint32_t kTrackLeaf = 16;   // rows a thread adds pairwise into one leaf of its tree
constexpr int kTrackLevels = 22;      // partial sums of a pairwise tree over up to 2^22 leaves per thread
inline uint32_t track_threads(uint32_t parents, uint32_t d) { return (uint64_t)parents * d > 8192u ? kTrackThreadsLarge : kTrackThreadsSmall; }

// Pairwise (tree) summation of a stream: level l holds the sum of a completed block of 2^l pushes; a push that finds its
// level taken adds the two blocks and carries the sum up, like a binary counter.  Every thread of the workgroup pushes
// the same number of times, so the tree's shape - and with it every rounding - depends on the row count alone.
struct TreeSum {
    float s[kTrackLevels];
    uint32_t n;
    __device__ __forceinline__ TreeSum() : n(0)
    {
#pragma unroll
        for (int l = 0; l < kTrackLevels; ++l) s[l] = 0.0f;
    }
    __device__ __forceinline__ void push(float v)
    {
        const uint32_t c = n++;
        bool open = true;
#pragma unroll
        for (int l = 0; l < kTrackLevels; ++l) {
            const bool taken = (c >> l) & 1u;
            const float up = s[l] + v;
            if (open && !taken) s[l] = v;
            if (open && taken) v = up;
            open = open && taken;
        }
    }
    // the blocks left over, smallest first
    __device__ __forceinline__ float total() const
    {
        float acc = 0.0f;
        bool has = false;
#pragma unroll
        for (int l = 0; l < kTrackLevels; ++l)
            if ((n >> l) & 1u) {
                acc = has ? s[l] + acc : s[l];
                has = true;
            }
        return acc;
    }
};

// the tree sum of x[(lane + k * lanes) * stride], k = 0, 1, ... while the row is below n: leaves of kTrackLeaf rows, added
// pairwise; rows past the end count as 0.0f (exact).  `groups` is the same for every thread.
__device__ __forceinline__ float track_column_sum(const float *__restrict__ x, uint32_t lane, uint32_t lanes, uint32_t stride,
                                                  uint32_t n, uint32_t groups, bool active)
{
    auto leaf = [&](uint32_t g) {
        float a[kTrackLeaf];
#pragma unroll
        for (uint32_t j = 0; j < kTrackLeaf; ++j) {
            const uint64_t r = (uint64_t)lane + (uint64_t)(g * kTrackLeaf + j) * lanes;
            a[j] = active && r < n ? x[r * stride] : 0.0f;
        }
#pragma unroll
        for (uint32_t w = kTrackLeaf / 2; w > 0; w >>= 1)
#pragma unroll
            for (uint32_t j = 0; j < w; ++j) a[j] = a[j] + a[j + w];
        return a[0];
    };
    if (groups == 1) return leaf(0); // (a tree of one leaf: what the cascade below returns, without running it)
    TreeSum sum;
    for (uint32_t g = 0; g < groups; ++g) sum.push(leaf(g));
    return sum.total();
}

// one wavefront joins the `count` (<= 1024) per-thread sums of a column: sixteen strided entries per lane pairwise, then
// a shuffle tree over the lanes.  Lane 0 holds the sum.
__device__ __forceinline__ float track_join(const float *col, uint32_t count, uint32_t lane)
{
    float a[16];
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) a[k] = lane + 64u * k < count ? col[lane + 64u * k] : 0.0f;
#pragma unroll
    for (uint32_t w = 8; w > 0; w >>= 1)
#pragma unroll
        for (uint32_t j = 0; j < w; ++j) a[j] = a[j] + a[j + w];
    float v = a[0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}

// meta[c] = {best-ever fitness bits, best-ever generation}; rows[c] = {values[16], steps[16]}; hist: [chunks][capacity]
// records of kTrackRecordFloats words (sots_gen_record).  slot == kTrackNoSlot: no history record this generation.
// blockDim.x = track_threads(parents, d).
__global__ __launch_bounds__(kTrackThreadsLarge) void k_track(const float *__restrict__ values, const float *__restrict__ steps,
                                                              const float *__restrict__ fitness, uint32_t p, uint32_t d, uint32_t parents,
                                                              uint32_t generation, uint32_t *__restrict__ meta, float *__restrict__ rows,
                                                              float *__restrict__ hist, uint32_t capacity, uint32_t slot)
{
    __shared__ float sm_fit[kTrackThreadsLarge];
    __shared__ float sm_step[kTrackThreadsLarge];
    const uint32_t c = blockIdx.x, t = threadIdx.x, threads = blockDim.x;
    const float *v = values + (size_t)c * p * d, *s = steps + (size_t)c * p * d, *f = fitness + (size_t)c * p;
    uint32_t *m = meta + 2u * (size_t)c;
    float *row = rows + (size_t)kTrackRowFloats * c;

    // best-ever: strictly better only, so a tie keeps the older record and NaN never wins
    const float f0 = f[0], worst = f[parents - 1];
    const float old = __uint_as_float(m[0]);
    const bool wins = f0 < old;
    const float best_ever = wins ? f0 : old;
    const bool record = slot != kTrackNoSlot;
    const uint32_t lanes = threads / d; // step sizes: thread t sums gene t % d over rows t / d, t / d + lanes, ...
    if (record) {
        // parent fitness: a strided tree sum per thread; step sizes: consecutive threads read consecutive floats
        const uint32_t per_f = (parents + threads - 1) / threads, per_s = (parents + lanes - 1) / lanes;
        sm_fit[t] = track_column_sum(f, t, threads, 1, parents, (per_f + kTrackLeaf - 1) / kTrackLeaf, true);
        const bool active = t < lanes * d;
        const uint32_t col = t % d, lane = t / d;
        const float sum = track_column_sum(s + col, lane, lanes, d, parents, (per_s + kTrackLeaf - 1) / kTrackLeaf, active);
        if (active) sm_step[col * lanes + lane] = sum;
    }
    __syncthreads(); // every thread holds the old record's fitness before thread 0 replaces it; the sums are in LDS
    if (wins) {
        if (t < d) row[t] = v[t];
        else if (t >= SOTS_MAX_DIMS && t < SOTS_MAX_DIMS + d) row[t] = s[t - SOTS_MAX_DIMS];
        if (t == 0) {
            m[0] = __float_as_uint(f0);
            m[1] = generation;
        }
    }
    if (!record) return;

    float *rec = hist + ((size_t)c * capacity + slot) * kTrackRecordFloats;
    const float count = (float)parents;
    const uint32_t wave = t / 64u, waves = threads / 64u, lane = t % 64u;
    // column d is the fitness; a wavefront joins the columns it is dealt
    for (uint32_t col = wave; col <= d; col += waves) {
        const float total = col < d ? track_join(sm_step + col * lanes, lanes, lane) : track_join(sm_fit, threads, lane);
        if (lane == 0) rec[col < d ? 8 + col : 4] = total / count;
    }
    if (t == 0) {
        reinterpret_cast<uint32_t *>(rec)[0] = generation;
        rec[1] = f0;
        rec[2] = best_ever;
        rec[3] = worst;
        rec[5] = 0.0f;
        rec[6] = 0.0f;
        rec[7] = 0.0f;
    }
    if (t >= d && t < SOTS_MAX_DIMS) rec[8 + t] = 0.0f;
}

// a cleared slot: fitness +inf, generation 0, zeroed rows
__global__ __launch_bounds__(256) void k_track_clear(uint32_t *__restrict__ meta, float *__restrict__ rows, uint32_t chunks)
{
    const uint32_t total = chunks * (2u + kTrackRowFloats);
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        if (e < 2u * chunks) meta[e] = e & 1u ? 0u : 0x7F800000u;
        else rows[e - 2u * chunks] = 0.0f;
    }
}

// ------------------------------------------------------------------------------------
// Chunk queue (sots_batch_queue_run): the run record of k_track (best-ever only) and the TURNOVER in one launch, a
// workgroup per slot, after every generation's sort.  A slot whose chunk's stop rule holds at one of the chunk's own
// check boundaries - or whose counter has reached max_generations - stores the chunk's result, draws the next unstarted
// chunk (ONE returning atomic on the queue head; nothing else passes between workgroups inside the launch, kernel
// boundaries on the stream order the rest), and is re-initialised for it: rows as k_init_population_seg draws them,
// record cleared, counter zeroed, target table rewritten from the stored targets.  With the queue empty the slot goes idle.
// values / steps / fitness: the half the sort has just written (the turnover writes the new chunk's rows there: it is the
// half the next generation's variation reads).
// CARRY (sots_batch_queue_set_carry): the chunks are cut into segments of q.segment_chunks; the head counts
// SEGMENTS, and inside a segment the slot takes chunk + 1 without touching it.  Such a successor keeps the retired
// chunk's rows where they lie: row 0 becomes the best-ever record (the `rec` words threads 0..31 hold), rows 1..R-1 stay
// as the sort left them, and the refill draws rows R..P-1 only - by local row index, so they are a fresh start's rows.
// Without CARRY the body is the kernel's as it was before carrying existed.
// ------------------------------------------------------------------------------------
template <int LOG2N>
__device__ __forceinline__ void queue_fill_x_table(float *__restrict__ image, const float *__restrict__ target, uint32_t slot,
                                                   uint32_t t, uint32_t threads)
{
    float *table = image + kSegHead + (size_t)slot * x_seg_stride<LOG2N>();
    for (uint32_t le = t; le < (uint32_t)(kWave * x_points<LOG2N>()); le += threads) x_seg_target_entry<LOG2N>(table, target, le);
}

template <bool CARRY>
__global__ __launch_bounds__(256) void k_queue_turnover(float *__restrict__ values, float *__restrict__ steps, float *__restrict__ fitness,
                                                        PopDims pd, uint32_t *__restrict__ meta, float *__restrict__ rows, QueueArgs q,
                                                        uint32_t global_generation)
{
    __shared__ uint32_t next_s;
    const uint32_t c = blockIdx.x, t = threadIdx.x, threads = blockDim.x, p = pd.p, d = pd.d;
    uint32_t *slot = q.slot_table + 2u * (size_t)c;
    const uint32_t chunk = slot[0];
    if (chunk == kQueueNoChunk) return; // idle (uniform over the workgroup)
    const uint32_t g = slot[1] + 1u;    // the chunk's own counter after this generation
    float *v = values + (size_t)c * p * d, *s = steps + (size_t)c * p * d, *f = fitness + (size_t)c * p;
    uint32_t *m = meta + 2u * (size_t)c;
    float *row = rows + (size_t)kTrackRowFloats * c;

    // best-ever, as k_track: strictly better only
    const float f0 = f[0], old = __uint_as_float(m[0]);
    const bool wins = f0 < old;
    const float ever_f = wins ? f0 : old;
    const uint32_t ever_g = wins ? g : m[1];
    float rec = 0.0f; // thread t < kTrackRowFloats: word t of the record's row {values[16], steps[16]} after this generation
    if (t < kTrackRowFloats) {
        const uint32_t j = t % SOTS_MAX_DIMS;
        rec = wins && j < d ? (t < SOTS_MAX_DIMS ? v[j] : s[j]) : row[t];
    }
    const bool look = q.check_interval != 0u && g % q.check_interval == 0u;
    const bool retire = g >= q.max_generations || (look && stop_rule_holds(q.target_fitness, q.stall_generations, ever_f, ever_g, g));
    __syncthreads(); // every thread holds the slot's words and the old record before anybody replaces them
    if (!retire) {
        if (wins) {
            if (t < kTrackRowFloats) row[t] = rec;
            if (t == 0) {
                m[0] = __float_as_uint(f0);
                m[1] = g;
            }
        }
        if (t == 0) slot[1] = g;
        return;
    }

    // ---- retire: the result (sots_chunk_result), the kept population ----
    float *res = q.results + (size_t)chunk * kQueueResultFloats;
    if (t == 0) {
        reinterpret_cast<uint32_t *>(res)[0] = g;
        reinterpret_cast<uint32_t *>(res)[1] = ever_g;
        res[2] = ever_f;
        res[3] = f0;
    }
    if (t < kTrackRowFloats) res[4 + t] = rec;
    if (t < SOTS_MAX_DIMS) res[4 + kTrackRowFloats + t] = t < d ? v[t] : 0.0f;
    if (chunk == q.keep_chunk) {
        for (uint32_t e = t; e < p * d; e += threads) {
            q.kept_values[e] = v[e];
            q.kept_steps[e] = s[e];
        }
        for (uint32_t e = t; e < p; e += threads) q.kept_fitness[e] = f[e];
    }
    // a successor: the next chunk of this chunk's segment
    const bool successor = CARRY && queue_has_successor(chunk, q.segment_chunks, q.num_chunks);
    if (t == 0) {
        atomicAdd(&q.state[1], 1u);                    // retired
        atomicMax(&q.state[2], global_generation);     // the loop generation of the last retirement
        if (!CARRY) {
            next_s = atomicAdd(&q.state[0], 1u);       // the queue head: the next unstarted chunk
        } else if (successor) {
            next_s = chunk + 1u;                       // inside a segment the head is not touched
        } else {
            const uint32_t seg = atomicAdd(&q.state[0], 1u); // the queue head: the next unstarted SEGMENT
            next_s = queue_segment_start(seg, q.segment_chunks, q.num_segments, kQueueNoChunk);
        }
    }
    __syncthreads(); // the draw is in LDS, and the old rows have been read
    const uint32_t next = next_s;
    if (next >= q.num_chunks) {
        if (t == 0) slot[0] = kQueueNoChunk;
        return;
    }

    // ---- refill: k_init_population_seg's draws for chunk first_chunk + next, a cleared record, the target table ----
    uint32_t fresh = 0u; // the first element drawn: a successor's rows 0..R-1 are carried (R <= numParents <= p)
    if (CARRY && successor) {
        fresh = q.carry_rows * d;
        if (t < kTrackRowFloats) { // row 0: the retired chunk's best-ever record
            const uint32_t j = t % SOTS_MAX_DIMS;
            if (j < d) (t < SOTS_MAX_DIMS ? v : s)[j] = rec;
        }
        for (uint32_t i = t; i < q.carry_rows; i += threads) f[i] = 0.0f;
    }
    for (uint32_t e = fresh + t; e < p * d; e += threads) {
        const uint32_t i = e / d, gene = e - i * d;
        const U4 rn = philox4x32_10(pd.gid_base + i, q.first_chunk + next, gene >> 2, kTagInit, pd.seed_lo, pd.seed_hi);
        const float u = draw_unit(u4_at(rn, gene & 3u));
        s[e] = 0.1f;
        v[e] = (u < 0.0f) ? -u : u;
        if (gene == 0) f[i] = 0.0f;
    }
    if (t < kTrackRowFloats) row[t] = 0.0f;
    if (t == 0) {
        m[0] = 0x7F800000u;
        m[1] = 0u;
        slot[0] = next;
        slot[1] = 0u;
    }
    const float *tg = q.targets + (size_t)next * q.half_bins;
    switch (q.x_log2n) {
    case 8: queue_fill_x_table<8>(q.seg_image, tg, c, t, threads); break;
    case 11: queue_fill_x_table<11>(q.seg_image, tg, c, t, threads); break;
    case 12: queue_fill_x_table<12>(q.seg_image, tg, c, t, threads); break;
    case 13: queue_fill_x_table<13>(q.seg_image, tg, c, t, threads); break;
    default: { // k_fft / k_fft_big: the N/2 bins
        float *table = q.seg_image + kSegHead + (size_t)c * q.half_bins;
        for (uint32_t k = t; k < q.half_bins; k += threads) table[k] = tg[k];
    }
    }
}

} // namespace

hipError_t launch_recombine_mutate_queue(hipStream_t st, const float *vin, const float *sin, float *vout, float *sout, const PopDims &pd,
                                         const MutateConsts &mc, const uint32_t *slot_table, uint32_t slots)
{
    k_recombine_mutate_queue<<<grid_for((uint64_t)slots * pd.p * pd.d, 256), 256, 0, st>>>(vin, sin, vout, sout, pd, mc, slot_table, slots);
    return hipGetLastError();
}

uint32_t queue_x_log2n(uint32_t log2n) { return x_from(log2n) && log2n != 10 ? log2n : 0u; }

hipError_t launch_queue_turnover(hipStream_t st, float *values, float *steps, float *fitness, const PopDims &pd, uint32_t *meta,
                                 float *rows, const QueueArgs &q, uint32_t global_generation, uint32_t slots)
{
    if (slots == 0 || pd.d == 0 || pd.d > SOTS_MAX_DIMS || q.num_chunks == 0 || q.max_generations == 0) return hipErrorInvalidValue;
    if (q.carry_rows) {
        // (the kernel trusts these: rows 0..R-1 lie inside the slot's population, and the segment arithmetic neither divides by 0 nor wraps)
        if (q.carry_rows > pd.p || q.segment_chunks == 0 || q.num_segments != (q.num_chunks - 1u) / q.segment_chunks + 1u) return hipErrorInvalidValue;
        k_queue_turnover<true><<<slots, 256, 0, st>>>(values, steps, fitness, pd, meta, rows, q, global_generation);
    } else {
        k_queue_turnover<false><<<slots, 256, 0, st>>>(values, steps, fitness, pd, meta, rows, q, global_generation);
    }
    return hipGetLastError();
}

hipError_t launch_track_clear(hipStream_t st, uint32_t *meta, float *rows, uint32_t chunks)
{
    k_track_clear<<<grid_for((uint64_t)chunks * (2u + kTrackRowFloats), 256), 256, 0, st>>>(meta, rows, chunks);
    return hipGetLastError();
}

hipError_t launch_track(hipStream_t st, const float *values, const float *steps, const float *fitness, uint32_t p, uint32_t d,
                        uint32_t parents, uint32_t generation, uint32_t chunks, uint32_t *meta, float *rows, float *hist,
                        uint32_t capacity, uint32_t slot)
{
    if (chunks == 0 || d == 0 || d > SOTS_MAX_DIMS || parents == 0 || parents > p) return hipErrorInvalidValue;
    if (slot != kTrackNoSlot && (!hist || slot >= capacity)) return hipErrorInvalidValue;
    k_track<<<chunks, track_threads(parents, d), 0, st>>>(values, steps, fitness, p, d, parents, generation, meta, rows, hist, capacity, slot);
    return hipGetLastError();
}

} // namespace sots

#if defined(SOTS_STAMP) || defined(SOTS_STAMP_ENDS)
extern "C" int sots_debug_stamps(unsigned long long *host, size_t n)
{
    if (n > 2 * 16384) n = 2 * 16384;
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(sots::g_stamps), n * sizeof(unsigned long long));
}
extern "C" int sots_debug_clear_stamps()
{
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(sots::g_stamps)) != hipSuccess) return -1;
    return (int)hipMemset(p, 0, sizeof(unsigned long long) * 2 * 16384);
}
#endif
