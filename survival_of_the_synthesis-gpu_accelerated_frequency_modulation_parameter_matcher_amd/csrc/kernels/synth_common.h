// synth_common.h -- what the synthesis kernels share: block lengths, the table read, the branch-free phase wraps, the
// tile constants and the shapes of the four voices.
#pragma once
#include "common.h"

// contraction: off (the translation unit's default: every per-sample operation is the reference's, unfused)
#pragma clang fp contract(off)
namespace sots { namespace {

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
//                For small populations a series chain is cut into two wavefronts (SPLIT, synth_lanes.h).
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

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
