// synth_lanes.h -- k_synth: every voice with a lane per individual, uncut or cut over two to four wavefronts (CutPlan),
// with the variation of the fused loop in front (HELP).
#pragma once
#include "common.h"
#include "stamps.h"
#include "variation.h"
#include "synth_common.h"

// contraction: off (the translation unit's default: every per-sample operation is the reference's, unfused)
#pragma clang fp contract(off)
namespace sots { namespace {

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

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
