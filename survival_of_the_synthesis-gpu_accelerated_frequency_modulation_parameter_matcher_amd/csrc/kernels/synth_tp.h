// synth_tp.h -- k_synth_tp: small populations, the time axis in the lanes (a scan wavefront and evaluation wavefronts per
// operator).
#pragma once
#include "common.h"
#include "variation.h"
#include "synth_common.h"

// contraction: off (the translation unit's default: every per-sample operation is the reference's, unfused)
#pragma clang fp contract(off)
namespace sots { namespace {

// ------------------------------------------------------------------------------------
// SMALL populations (a few individuals per CU), every voice: the time axis in the lanes.
//
// k_synth (synth_lanes.h) puts an individual in a lane and pays its ten to twenty vector instructions per sample and operator whether
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

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
