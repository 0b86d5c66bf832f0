// sots_render_graph_continuous.hip -- phase-continuous rendering of a parameter track of the operator-graph voice
// (sots_render_graph_continuous): the track as ONE voice whose oscillators never restart, for any
// feed-forward graph of 2 to 8 operators without feedback.
//
// As in sots_render_continuous.hip the phases are 32-bit words, unsigned 15.17 fixed point, and an operator's phase is the
// exclusive prefix sum of its increments: reduce (a tile's increments summed), scan (the tile totals, one workgroup per
// operator, on top of the carry of the pass before), apply (the increments again, scanned inside the tile on top of its
// base) - three plain launches in stream order.  No workgroup waits for another: no look-back, no flags, no grid barrier.
// What differs: operator j's increment at sample n reads the phases at n of the operators i < j that modulate it, whichever
// they are, so
//   * the launches go by LEVEL of the graph (graph_levels, sots_rules.h): the operators of a level do not read each other and
//     sit in grid.y of the level's three launches.  A chain of 8 is 8 levels, a sum of 8 unmodulated carriers is one;
//   * every operator has a phase buffer of its own, a word per sample of the pass, which the later levels and the mix read;
//   * the topology and the packed 3-bit waveform codes are scalar kernel arguments, as in k_synth_graph: the loop over an
//     operator's set modulator bits and the branch on a modulator's code are wavefront-uniform;
//   * a last launch, mix, reads the carriers' words and adds their outputs in ascending order.
// A modulator's output is made from its phase word where it is read (shape(w, Phi >> 17) A): a stored output would be a
// second buffer per operator, making it again is one table read from LDS and three products.  The increments are made twice
// (reduce and apply) and not stored, as in 4.10.  A sum starts from -0.0f, for which -0 + x == x bit for bit, and only
// operators whose bit is set are added to it: a cleared bit is skipped, as the definition says.
// Every fp32 expression is the definition's (include/sots_hip.h), uncontracted; tests/_render_graph_continuous_model.py
// states the whole in NumPy.
#include "sots_render.h"
#include "sots_render_scan.h"      // cont_fix, cont_load_table, cont_block_scan, k_cont_scan
#include "sots_render_graph_dev.h" // GraphTopo, gcont_sample, gcont_param, gcont_shape, gcont_indices, gcont_samples
#include "sots_rules.h"            // graph_levels, graph_level_reads_table

#pragma clang fp contract(off)

namespace sots {

namespace {

// The four increments of operator j in this lane's quad (0 behind the pass's end).  first: the quad's first pass sample.
template <bool TABLE>
__device__ inline void gcont_quad(const GraphContPass &ps, const GraphTopo &tp, uint32_t j, uint32_t first, const float *tab, uint32_t inc[4])
{
    const float c = (float)kWavetableSize / (float)SOTS_SAMPLE_RATE;
    const uint32_t d = 2u * tp.ops;
    GraphSample sm[4];
    gcont_samples(ps, d, first, sm);
    float cur[4] = {-0.0f, -0.0f, -0.0f, -0.0f};
    const uint32_t mods = tp.modulators[j];
    for (uint32_t m = mods; m != 0u; m &= m - 1u) { // set bits in ascending i: wavefront-uniform
        const uint32_t i = (uint32_t)__builtin_ctz(m);
        uint32_t at[4];
        float tv[4];
        gcont_indices(ps, i, first, at);
        gcont_shape<TABLE>(tp.shapes >> (3u * i) & 7u, at, tab, tv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float level = gcont_param(ps, sm[e], d, 2u * i) * gcont_param(ps, sm[e], d, 2u * i + 1u); // A_i = f_i a_i: a modulator
            cur[e] = cur[e] + tv[e] * level;
        }
    }
#pragma unroll
    for (uint32_t e = 0; e < 4u; ++e) {
        const float f = gcont_param(ps, sm[e], d, 2u * j);
        const float x = mods != 0u ? cur[e] + f : f;
        inc[e] = first + e < ps.count ? cont_fix(c * x) : 0u;
    }
}

// grid (tiles by stride, operators of the level); level_ops: the level's operators, 3 bits each, in grid.y order
template <bool TABLE> __global__ __launch_bounds__(kContThreads) void k_gcont_reduce(GraphContPass ps, GraphTopo tp, uint32_t level_ops, uint32_t tiles)
{
    __shared__ float tab_s[TABLE ? kWavetableSize : 4];
    __shared__ uint32_t wtot[2][kContWaves];
    if constexpr (TABLE) cont_load_table(tab_s, ps.wavetable);
    const uint32_t j = level_ops >> (3u * blockIdx.y) & 7u;
    uint32_t *totals = ps.words + ps.lay.totals + (size_t)blockIdx.y * tiles;
    uint32_t parity = 0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, parity ^= 1u) {
        uint32_t inc[4];
        gcont_quad<TABLE>(ps, tp, j, tile * kContTile + 4u * threadIdx.x, tab_s, inc);
        uint32_t sum = inc[0] + inc[1] + inc[2] + inc[3];
#pragma unroll
        for (uint32_t d = 32; d > 0u; d >>= 1) sum += __shfl_xor(sum, d);
        if ((threadIdx.x & 63u) == 0u) wtot[parity][threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t all = 0;
#pragma unroll
            for (int w = 0; w < kContWaves; ++w) all += wtot[parity][w];
            totals[tile] = all;
        }
    }
}

// grid as above: the operators' phase words
template <bool TABLE> __global__ __launch_bounds__(kContThreads) void k_gcont_apply(GraphContPass ps, GraphTopo tp, uint32_t level_ops, uint32_t tiles)
{
    __shared__ float tab_s[TABLE ? kWavetableSize : 4];
    __shared__ uint32_t wtot[2][kContWaves];
    if constexpr (TABLE) cont_load_table(tab_s, ps.wavetable);
    const uint32_t j = level_ops >> (3u * blockIdx.y) & 7u;
    const uint32_t *bases = ps.words + ps.lay.totals + (size_t)blockIdx.y * tiles;
    uint32_t *buf = ps.words + (size_t)j * ps.lay.stride;
    uint32_t parity = 0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, parity ^= 1u) {
        const uint32_t first = tile * kContTile + 4u * threadIdx.x;
        uint32_t inc[4], total;
        gcont_quad<TABLE>(ps, tp, j, first, tab_s, inc);
        uint32_t phi = bases[tile] + cont_block_scan(inc[0] + inc[1] + inc[2] + inc[3], wtot[parity], total);
        uint32_t w[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) w[e] = phi, phi += inc[e];
        if (first + 4u <= ps.count) {
            *reinterpret_cast<uint4 *>(buf + first) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e)
                if (first + e < ps.count) buf[first + e] = w[e];
        }
    }
}

// grid (tiles by stride): the carriers' outputs added in ascending j, divided by their number where there are several
template <bool TABLE> __global__ __launch_bounds__(kContThreads) void k_gcont_mix(GraphContPass ps, GraphTopo tp, uint32_t tiles)
{
    __shared__ float tab_s[TABLE ? kWavetableSize : 4];
    if constexpr (TABLE) cont_load_table(tab_s, ps.wavetable);
    const uint32_t d = 2u * tp.ops;
    const uint32_t heard = (uint32_t)__builtin_popcount(tp.carriers);
    const float heard_f = (float)heard;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t first = tile * kContTile + 4u * threadIdx.x;
        if (first >= ps.count) continue; // (no barrier below)
        GraphSample sm[4];
        gcont_samples(ps, d, first, sm);
        float acc[4] = {-0.0f, -0.0f, -0.0f, -0.0f};
        for (uint32_t m = tp.carriers; m != 0u; m &= m - 1u) {
            const uint32_t j = (uint32_t)__builtin_ctz(m);
            uint32_t at[4];
            float tv[4];
            gcont_indices(ps, j, first, at);
            gcont_shape<TABLE>(tp.shapes >> (3u * j) & 7u, at, tab_s, tv);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = acc[e] + tv[e] * gcont_param(ps, sm[e], d, 2u * j + 1u); // A_j = a_j: a carrier
        }
        if (heard > 1u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = acc[e] / heard_f;
        }
        if (first + 4u <= ps.count) {
            *reinterpret_cast<float4 *>(ps.out + first) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e)
                if (first + e < ps.count) ps.out[first + e] = acc[e];
        }
    }
}

template <bool TABLE>
hipError_t gcont_level(hipStream_t st, const GraphContPass &ps, const GraphTopo &tp, uint32_t level_ops, uint32_t in_level, uint32_t first_slot,
                       uint32_t tiles, uint32_t num_cus)
{
    // With the 128 KiB table in LDS: one workgroup per compute unit, looping over its tiles; without it, two.
    const uint32_t resident = TABLE ? num_cus : 2u * num_cus;
    const uint32_t gx = tiles < resident ? tiles : resident;
    k_gcont_reduce<TABLE><<<dim3(gx, in_level), kContThreads, 0, st>>>(ps, tp, level_ops, tiles);
    if (hipError_t e = hipGetLastError()) return e;
    k_cont_scan<<<in_level, kContThreads, 0, st>>>(ps.words + ps.lay.totals, ps.words + ps.lay.carry + first_slot, tiles);
    if (hipError_t e = hipGetLastError()) return e;
    k_gcont_apply<TABLE><<<dim3(gx, in_level), kContThreads, 0, st>>>(ps, tp, level_ops, tiles);
    return hipGetLastError();
}

} // namespace

hipError_t launch_graph_continuous_pass(hipStream_t st, const sots_voice_graph &graph, const uint32_t waveforms[8], const GraphContPass &ps,
                                        uint32_t num_cus)
{
    if (!ps.values || !ps.wavetable || !ps.words || !ps.out || ps.num_rows == 0 || ps.hop == 0 || ps.hop > 2u * ps.half_n) return hipErrorInvalidValue;
    if (voice_graph_check(&graph)) return hipErrorInvalidValue;
    if (ps.count == 0) return hipSuccess;
    const uint32_t ops = graph.num_operators;
    // what the kernels' 32-bit indices and the scratch layout rest on
    if (ps.count > graph_continuous_max_pass(ops) || ps.count > ps.lay.stride || (uint64_t)ps.n0 + ps.count > (1ull << 31)) return hipErrorInvalidValue;
    const uint32_t tiles = (ps.count + kContTile - 1u) / kContTile;
    if (tiles > ps.lay.tiles || tiles > (uint32_t)kContThreads || num_cus == 0) return hipErrorInvalidValue;
    if (ps.lay.totals < (size_t)ops * ps.lay.stride || ps.lay.carry < ps.lay.totals + (size_t)8u * ps.lay.tiles) return hipErrorInvalidValue;
    GraphTopo tp{};
    tp.ops = ops, tp.carriers = graph.carriers;
    uint32_t codes[8];
    for (uint32_t j = 0; j < 8u; ++j) {
        codes[j] = j < ops ? waveforms[j] & 7u : 0u;
        tp.modulators[j] = graph.modulators[j];
    }
    tp.shapes = pack_waveforms(codes);
    const GraphLevels lv = graph_levels(graph);
    for (uint32_t l = 0; l < lv.count; ++l) {
        const uint32_t in_level = lv.first[l + 1u] - lv.first[l];
        uint32_t level_ops = 0;
        for (uint32_t s = 0; s < in_level; ++s) level_ops |= lv.ops[lv.first[l] + s] << (3u * s);
        const hipError_t e = graph_level_reads_table(graph, lv, codes, l)
                                 ? gcont_level<true>(st, ps, tp, level_ops, in_level, lv.first[l], tiles, num_cus)
                                 : gcont_level<false>(st, ps, tp, level_ops, in_level, lv.first[l], tiles, num_cus);
        if (e != hipSuccess) return e;
    }
    bool table = false;
    for (uint32_t j = 0; j < ops; ++j) table = table || ((graph.carriers >> j & 1u) && waveform_reads_table(codes[j]));
    const uint32_t resident = table ? num_cus : 2u * num_cus, gx = tiles < resident ? tiles : resident;
    if (table) k_gcont_mix<true><<<gx, kContThreads, 0, st>>>(ps, tp, tiles);
    else k_gcont_mix<false><<<gx, kContThreads, 0, st>>>(ps, tp, tiles);
    return hipGetLastError();
}

} // namespace sots
