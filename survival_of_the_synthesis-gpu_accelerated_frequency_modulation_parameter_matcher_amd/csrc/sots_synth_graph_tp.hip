// sots_synth_graph_tp.hip -- k_synth_graph_tp: the operator-graph voice for SMALL populations, the time axis in the lanes
// (after k_synth_tp, kernels/synth_tp.h).  The voice is defined in include/sots_hip.h (sots_voice_graph);
// every value sees the operations of the sample-by-sample order, unfused (-ffp-contract=off), so the audio is
// k_synth_graph's (sots_synth_graph.hip) and the NumPy model's bit for bit.
//
// Only an operator's PHASE is a recurrence over the samples.  Per operator j and block of 64 samples:
//   * its SCAN wavefront first, lane = SAMPLE and only where j is modulated, forms the 64 increments c (cur + f_j) of one
//     individual after another - cur summed from -0.0f over the set bits of modulators[j] in ascending i, a cleared bit
//     skipped - then, lane = INDIVIDUAL, turns them into the 64 phases in their place: the definition's additions and wraps
//     in its order (the lower wrap for a modulated operator only);
//   * its one or two EVALUATION wavefronts, lane = SAMPLE, one tick later take individual after individual: the index
//     (the clamp decided on the float), the shaped table value, times the operator's level.  The output goes into the
//     operator's RING of blocks, which the scans of the operators it modulates - or the mixer - read at their own tick.
//     The MIXER is the evaluator of the carrier that runs last: it sums the carriers from -0.0f in ascending j, its own
//     value from its register and the others from their rings, divides by their count where there are several, and stores
//     a whole 256-byte piece of an audio row per instruction.
// One workgroup barrier per tick.  When each operator runs, how deep its ring is and where its buffers lie in the 31 KiB
// beside the table is the PLAN (graph_tp_plan, sots_rules.h): host code, computed once, handed over as an argument.
// The masks, a wavefront's operator and its role are wavefront-uniform: one kernel for every operator count, in two
// instantiations, all sine and shaped.  No scratch, no atomics, no workgroup waits for another.
#include "kernels/common.h"
#include "kernels/synth_common.h"

#pragma clang fp contract(off)
namespace sots {
namespace {

struct GraphTpMasks {
    uint32_t carriers;
    uint32_t modulators[8];
};
static_assert(kGraphTpRow % 4 == 0, "the scan reads and writes 16 bytes at a time");

template <bool SHAPED>
__global__ __launch_bounds__(1024) void k_synth_graph_tp(const float *__restrict__ values, const float *__restrict__ wavetable,
                                                         float *__restrict__ audio, SynthParams sp, GraphTpMasks gm, GraphTpPlan plan,
                                                         uint32_t p_len, uint32_t n, uint32_t pitch, uint32_t per_group, uint32_t groups,
                                                         uint32_t shapes)
{
    __shared__ float tab[kWavetableSize];
    __shared__ __attribute__((aligned(16))) float buf[kGraphTpLdsBytes / 4]; // phases and rings: plan.phase_off, plan.ring_off
    request_wavetable(tab, wavetable);
    const float wf = (float)kWavetableSize;
    const float c = (float)kWavetableSize / (float)SOTS_SAMPLE_RATE;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t ops = plan.ops, ne = plan.evaluators, cap = plan.capacity;
    const bool scans = wave < ops; // the first OPS wavefronts scan, the others evaluate (ne per operator)
    const uint32_t j = scans ? wave : (wave - ops) / ne, ev = scans ? 0u : (wave - ops) % ne;
    const uint32_t block_floats = cap * kGraphTpRow; // one block of every individual of the workgroup
    // this wavefront's operator: its entries of the argument structs, picked with compile-time indices (the structs stay in
    // scalar registers; an index known only at run time would put them in memory)
    uint32_t mods = 0, my_tick = 0, my_depth = 0, my_phase_off = 0, my_ring_off = 0;
    float fmin_j = 0.0f, fmax_j = 0.0f, amin_j = 0.0f, amax_j = 0.0f;
    static_for<0, 8>([&](auto i_tag) {
        constexpr int I = decltype(i_tag)::value;
        if (j == (uint32_t)I) {
            mods = gm.modulators[I], my_tick = plan.tick_of[I], my_depth = plan.depth[I];
            my_phase_off = plan.phase_off[I], my_ring_off = plan.ring_off[I];
            fmin_j = sp.pmin[2 * I], fmax_j = sp.pmax[2 * I], amin_j = sp.pmin[2 * I + 1], amax_j = sp.pmax[2 * I + 1];
        }
    });
    if (!scans) my_tick += 1u;
    float *const my_phase = buf + my_phase_off;
    float *const my_ring = buf + my_ring_off;
    const bool carrier = gm.carriers >> j & 1u, mixer = j == plan.mixer;
    const uint32_t code = SHAPED ? shapes >> (3u * j) & 7u : 0u;
    const float carriers_f = (float)plan.num_carriers;

    // table[clamp((int)pos, 0, W-1)], the clamp decided on the float: NaN and negatives give entry 0
    auto index_of = [&](float pos) { return (uint32_t)fminf(fmaxf(pos, 0.0f), wf - 1.0f); };
    auto lane_value = [](float v, uint32_t of) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)of)); };
    wavetable_ready();

    const uint32_t blocks = n / kWave, ticks = blocks + plan.lag;
    for (uint32_t group = blockIdx.x; group < groups; group += gridDim.x) {
        const uint32_t first = group * per_group;
        const uint32_t count = p_len - first < per_group ? p_len - first : per_group; // individuals here (1 .. capacity)
        // lane i < count: individual first + i; this operator's frequency and level as k_synth_graph makes them
        const uint32_t ind = first + (lane < count ? lane : count - 1u);
        const float f = fmin_j + values[(size_t)ind * (2u * ops) + 2u * j] * (fmax_j - fmin_j);
        const float a = amin_j + values[(size_t)ind * (2u * ops) + 2u * j + 1u] * (amax_j - amin_j);
        const float amp = carrier ? a : f * a;
        const float inc0 = c * (-0.0f + f); // (an unmodulated operator's increment: cur stays -0.0f)
        float pos = 0.0f;                   // (scan wavefronts) this operator's phase of individual `lane`
        uint32_t slot[8] = {0, 0, 0, 0, 0, 0, 0, 0}, my_slot = 0; // block mod ring depth, per operator and of this one

        for (uint32_t tick = 0; tick < ticks; ++tick) {
            const uint32_t k = tick - my_tick; // this wavefront's block (wraps to a large number before its first)
            if (k < blocks) {
                float *const rows = my_phase + (k & 1u) * block_floats;
                if (scans) {
                    if (mods) {
                        // lane = sample: the increments, four individuals at a time
                        for (uint32_t i0 = 0; i0 < count; i0 += 4u) {
                            float cur[4] = {-0.0f, -0.0f, -0.0f, -0.0f};
                            static_for<0, 7>([&](auto i_tag) {
                                constexpr int I = decltype(i_tag)::value;
                                if (mods >> I & 1u) {
                                    const float *src = buf + plan.ring_off[I] + slot[I] * block_floats + lane;
#pragma unroll
                                    for (uint32_t q = 0; q < 4; ++q) cur[q] += src[(i0 + q < count ? i0 + q : i0) * kGraphTpRow];
                                }
                            });
#pragma unroll
                            for (uint32_t q = 0; q < 4; ++q) {
                                const uint32_t i = i0 + q;
                                if (i >= count) break;
                                rows[i * kGraphTpRow + lane] = c * (cur[q] + lane_value(f, i));
                            }
                        }
                        __builtin_amdgcn_wave_barrier(); // (one wavefront: its LDS accesses complete in order)
                        asm volatile("" ::: "memory");
                    }
                    if (lane < count) { // lane = individual: phases in place of increments, four samples per access
                        float4 *row = reinterpret_cast<float4 *>(rows + lane * kGraphTpRow);
                        if (!mods) {
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
                    float *const out = my_ring + my_slot * block_floats + lane;
                    constexpr uint32_t H = (uint32_t)kWavetableSize / 2u, Q = (uint32_t)kWavetableSize / 4u;
                    // four individuals at a time: their phases, then their table values, are asked for together
                    for (uint32_t i0 = 4u * ev; i0 < count; i0 += 4u * ne) {
                        uint32_t at[4];
                        float t[4];
#pragma unroll
                        for (uint32_t q = 0; q < 4; ++q) at[q] = index_of(rows[(i0 + q < count ? i0 + q : i0) * kGraphTpRow + lane]);
                        auto read = [&](auto shape) {
#pragma unroll
                            for (uint32_t q = 0; q < 4; ++q) t[q] = shape(at[q]);
                        };
                        if constexpr (SHAPED) { // the shapes of sots_set_voice_waveforms, each decided on the integer index
                            switch (code) {
                            case SOTS_WAVE_HALF: read([&](uint32_t i) { return i < H ? tab[i] : 0.0f; }); break;
                            case SOTS_WAVE_ABS: read([&](uint32_t i) { return fabsf(tab[i]); }); break;
                            case SOTS_WAVE_PULSE: read([&](uint32_t i) { return (i & Q) == 0 ? fabsf(tab[i]) : 0.0f; }); break;
                            case SOTS_WAVE_EVEN: read([&](uint32_t i) { return i < H ? tab[2u * i] : 0.0f; }); break;
                            case SOTS_WAVE_ABS_EVEN: read([&](uint32_t i) { return i < H ? fabsf(tab[2u * i]) : 0.0f; }); break;
                            case SOTS_WAVE_SQUARE: read([&](uint32_t i) { return i < H ? 1.0f : -1.0f; }); break;
                            case SOTS_WAVE_SAW: read([&](uint32_t i) { return (float)i * 0x1p-14f - 1.0f; }); break;
                            default: read([&](uint32_t i) { return tab[i]; }); break;
                            }
                        } else {
                            read([&](uint32_t i) { return tab[i]; });
                        }
#pragma unroll
                        for (uint32_t q = 0; q < 4; ++q) {
                            const uint32_t i = i0 + q;
                            if (i >= count) break;
                            const float o = t[q] * lane_value(amp, i);
                            if (!mixer) {
                                out[i * kGraphTpRow] = o;
                                continue;
                            }
                            float y = -0.0f;
                            static_for<0, 8>([&](auto i_tag) {
                                constexpr int I = decltype(i_tag)::value;
                                if (gm.carriers >> I & 1u)
                                    y += j == (uint32_t)I ? o : buf[plan.ring_off[I] + slot[I] * block_floats + i * kGraphTpRow + lane];
                            });
                            if (plan.num_carriers > 1u) y = y / carriers_f;
                            audio[(size_t)(first + i) * pitch + k * kWave + lane] = y;
                        }
                    }
                }
                static_for<0, 8>([&](auto i_tag) {
                    constexpr int I = decltype(i_tag)::value;
                    slot[I] = slot[I] + 1u == plan.depth[I] ? 0u : slot[I] + 1u;
                });
                my_slot = my_slot + 1u == my_depth ? 0u : my_slot + 1u;
            }
            __syncthreads();
        }
    }
}

} // namespace

hipError_t launch_synth_graph_tp(hipStream_t st, const sots_voice_graph &graph, const float *values, const float *wavetable, float *audio,
                                 const SynthParams &sp, uint32_t p, uint32_t log2n, uint32_t pitch, uint32_t num_cus, uint32_t waveforms)
{
    const GraphTpPlan plan = graph_tp_plan(graph);
    if (p == 0 || log2n < 8 || pitch < (1u << log2n) || plan.capacity == 0) return hipErrorInvalidValue;
    GraphTpMasks gm;
    gm.carriers = graph.carriers;
    for (int j = 0; j < 8; ++j) gm.modulators[j] = graph.modulators[j];
    // one workgroup per CU (the table) takes its share of the rows, up to the plan's capacity; beyond that a launch has
    // more groups of rows than CUs and the workgroups loop over them
    const uint32_t n = 1u << log2n, cus = num_cus ? num_cus : 256;
    const uint32_t share = (p + cus - 1) / cus, per_group = share < plan.capacity ? share : plan.capacity;
    const uint32_t groups = (p + per_group - 1) / per_group, grid = groups < cus ? groups : cus;
    const uint32_t threads = plan.ops * (1u + plan.evaluators) * kWave;
    // (checked codes hold nothing beyond the operators: all sine is 0 and launches the kernel that reads no codes)
    const uint32_t shapes = graph.num_operators < 8 ? waveforms & ((1u << 3 * graph.num_operators) - 1u) : waveforms & 0xFFFFFFu;
    if (shapes) k_synth_graph_tp<true><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, gm, plan, p, n, pitch, per_group, groups, shapes);
    else k_synth_graph_tp<false><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, gm, plan, p, n, pitch, per_group, groups, 0u);
    return hipGetLastError();
}

} // namespace sots
