// sots_render_graph_feedback.hip -- phase-continuous rendering of a parameter track of the operator-graph voice with feedback
// operators (sots_render_graph_feedback).
//
// Feedback never touches a phase: every Phi_j is still the exclusive prefix sum of its increments, so the levels, the three
// launches per level and the phase buffers are those of sots_render_graph_continuous.hip (4.16).  What an operator with
// beta_j != 0 adds is ONE chain over the samples, which turns its finished phase words and the constant B_j into its shaped
// values t_j(n) = shape(w_j, (Phi_j(n) + fix(B_j (t_j(n-1) + t_j(n-2)) / 2)) >> 17):
//   * after a level's reduce / scan / apply, one chain launch with the level's feedback operators in the grid reads Phi_j of
//     the pass and writes a float buffer t_j of the pass; only feedback operators have such a buffer;
//   * reduce, apply and mix take the value of a flagged modulator or carrier from its t buffer, decided by a scalar mask
//     argument (wavefront-uniform), and make every other operator's from its phase word as in 4.16;
//   * between passes an operator carries its end phase and h1, h2.
// The chain has two forms with the same bits.  Serial: one wavefront per operator; the phase words come a block at a time by
// coalesced loads, the next block in flight while lane 0 runs the chain over the current one out of LDS, and t leaves a block
// at a time.  Relaxation: one workgroup per operator walks tiles of 1024 samples in order; a tile starts from the
// feed-forward values, every sweep recomputes every sample from its two predecessors in the other copy, and the tile is done
// at a sweep that changed no lane's bits - it then satisfies the recurrence everywhere, and the recurrence has one solution.
// Sweep k makes at least the first k samples final, so after relax_cap sweeps lane 0 finishes the tile from sample relax_cap.
// No workgroup waits for another, no atomics, no scratch.  Every fp32 expression is the definition's (include/sots_hip.h),
// uncontracted; tests/_render_graph_feedback_model.py states both forms in NumPy.
#include "sots_render.h"
#include "sots_render_scan.h"      // cont_fix, cont_load_table, cont_block_scan, k_cont_scan
#include "sots_render_graph_dev.h" // GraphTopo, gcont_sample, gcont_param, gcont_shape, gcont_indices, gcont_samples
#include "sots_rules.h"            // graph_levels, waveform_reads_table, graph_feedback_max_pass

#pragma clang fp contract(off)

namespace sots {

namespace {

constexpr uint32_t kRelaxTile = 1024;  // samples per tile of the relaxation: one per lane
constexpr uint32_t kSerialBlock = 256; // phase words per block of the serial form: a quad per lane of one wavefront
static_assert(kRelaxTile == (uint32_t)kContThreads, "a relaxation tile is one sample per lane");

// the t buffer's position among the flagged operators, in ascending j
__device__ inline uint32_t gfb_slot(uint32_t mask, uint32_t j) { return (uint32_t)__builtin_popcount(mask & ((1u << j) - 1u)); }
__device__ inline float *gfb_tbuf(const GraphFbPass &ps, uint32_t j)
{
    return reinterpret_cast<float *>(ps.g.words + ps.tbuf) + (size_t)gfb_slot(ps.fb_mask, j) * ps.g.lay.stride;
}
__device__ inline float *gfb_hist(const GraphFbPass &ps, uint32_t j)
{
    return reinterpret_cast<float *>(ps.g.words + ps.hist) + 2u * gfb_slot(ps.fb_mask, j);
}
__device__ inline bool gfb_reads_table(uint32_t w) { return w != SOTS_WAVE_SQUARE && w != SOTS_WAVE_SAW; }

// shape(w, i) of one index: gcont_shape's own cases
template <bool TABLE> __device__ inline float gfb_shape(uint32_t w, uint32_t at, const float *tab)
{
    const uint32_t a4[4] = {at, at, at, at};
    float tv[4];
    gcont_shape<TABLE>(w, a4, tab, tv);
    return tv[0];
}
// t_j(n) from the phase word and the two shaped values before it
template <bool TABLE> __device__ inline float gfb_step(uint32_t w, uint32_t phi, float scaled, float h1, float h2, const float *tab)
{
    const float g = (h1 + h2) * 0.5f;
    const uint32_t z = phi + cont_fix(scaled * g);
    return gfb_shape<TABLE>(w, z >> 17, tab);
}

// this lane's quad of operator i's shaped values: from its t buffer where i is flagged (0 behind the pass's end), else from
// its phase words
template <bool TABLE>
__device__ inline void gfb_values(const GraphFbPass &ps, const GraphTopo &tp, uint32_t i, uint32_t first, const float *tab, float tv[4])
{
    if (ps.fb_mask >> i & 1u) { // a kernel argument: wavefront-uniform
        const float *buf = gfb_tbuf(ps, i);
        tv[0] = tv[1] = tv[2] = tv[3] = 0.0f;
        if (first + 4u <= ps.g.count) {
            const float4 q = *reinterpret_cast<const float4 *>(buf + first);
            tv[0] = q.x, tv[1] = q.y, tv[2] = q.z, tv[3] = q.w;
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e)
                if (first + e < ps.g.count) tv[e] = buf[first + e];
        }
        return;
    }
    uint32_t at[4];
    gcont_indices(ps.g, i, first, at);
    gcont_shape<TABLE>(tp.shapes >> (3u * i) & 7u, at, tab, tv);
}

// The four increments of operator j in this lane's quad (0 behind the pass's end): gcont_quad of 4.16 with gfb_values
template <bool TABLE>
__device__ inline void gfb_quad(const GraphFbPass &ps, const GraphTopo &tp, uint32_t j, uint32_t first, const float *tab, uint32_t inc[4])
{
    const float c = (float)kWavetableSize / (float)SOTS_SAMPLE_RATE;
    const uint32_t d = 2u * tp.ops;
    GraphSample sm[4];
    gcont_samples(ps.g, d, first, sm);
    float cur[4] = {-0.0f, -0.0f, -0.0f, -0.0f};
    const uint32_t mods = tp.modulators[j];
    for (uint32_t m = mods; m != 0u; m &= m - 1u) { // set bits in ascending i: wavefront-uniform
        const uint32_t i = (uint32_t)__builtin_ctz(m);
        float tv[4];
        gfb_values<TABLE>(ps, tp, i, first, tab, tv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float level = gcont_param(ps.g, sm[e], d, 2u * i) * gcont_param(ps.g, sm[e], d, 2u * i + 1u); // A_i = f_i a_i: a modulator
            cur[e] = cur[e] + tv[e] * level;
        }
    }
#pragma unroll
    for (uint32_t e = 0; e < 4u; ++e) {
        const float f = gcont_param(ps.g, sm[e], d, 2u * j);
        const float x = mods != 0u ? cur[e] + f : f;
        inc[e] = first + e < ps.g.count ? cont_fix(c * x) : 0u;
    }
}

// grid (tiles by stride, operators of the level); level_ops: the level's operators, 3 bits each, in grid.y order
template <bool TABLE> __global__ __launch_bounds__(kContThreads) void k_gfb_reduce(GraphFbPass ps, GraphTopo tp, uint32_t level_ops, uint32_t tiles)
{
    __shared__ float tab_s[TABLE ? kWavetableSize : 4];
    __shared__ uint32_t wtot[2][kContWaves];
    if constexpr (TABLE) cont_load_table(tab_s, ps.g.wavetable);
    const uint32_t j = level_ops >> (3u * blockIdx.y) & 7u;
    uint32_t *totals = ps.g.words + ps.g.lay.totals + (size_t)blockIdx.y * tiles;
    uint32_t parity = 0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, parity ^= 1u) {
        uint32_t inc[4];
        gfb_quad<TABLE>(ps, tp, j, tile * kContTile + 4u * threadIdx.x, tab_s, inc);
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
template <bool TABLE> __global__ __launch_bounds__(kContThreads) void k_gfb_apply(GraphFbPass ps, GraphTopo tp, uint32_t level_ops, uint32_t tiles)
{
    __shared__ float tab_s[TABLE ? kWavetableSize : 4];
    __shared__ uint32_t wtot[2][kContWaves];
    if constexpr (TABLE) cont_load_table(tab_s, ps.g.wavetable);
    const uint32_t j = level_ops >> (3u * blockIdx.y) & 7u;
    const uint32_t *bases = ps.g.words + ps.g.lay.totals + (size_t)blockIdx.y * tiles;
    uint32_t *buf = ps.g.words + (size_t)j * ps.g.lay.stride;
    uint32_t parity = 0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, parity ^= 1u) {
        const uint32_t first = tile * kContTile + 4u * threadIdx.x;
        uint32_t inc[4], total;
        gfb_quad<TABLE>(ps, tp, j, first, tab_s, inc);
        uint32_t phi = bases[tile] + cont_block_scan(inc[0] + inc[1] + inc[2] + inc[3], wtot[parity], total);
        uint32_t w[4];
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) w[e] = phi, phi += inc[e];
        if (first + 4u <= ps.g.count) {
            *reinterpret_cast<uint4 *>(buf + first) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e)
                if (first + e < ps.g.count) buf[first + e] = w[e];
        }
    }
}

// grid (tiles by stride): the carriers' outputs added in ascending j, divided by their number where there are several
template <bool TABLE> __global__ __launch_bounds__(kContThreads) void k_gfb_mix(GraphFbPass ps, GraphTopo tp, uint32_t tiles)
{
    __shared__ float tab_s[TABLE ? kWavetableSize : 4];
    if constexpr (TABLE) cont_load_table(tab_s, ps.g.wavetable);
    const uint32_t d = 2u * tp.ops;
    const uint32_t heard = (uint32_t)__builtin_popcount(tp.carriers);
    const float heard_f = (float)heard;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t first = tile * kContTile + 4u * threadIdx.x;
        if (first >= ps.g.count) continue; // (no barrier below)
        GraphSample sm[4];
        gcont_samples(ps.g, d, first, sm);
        float acc[4] = {-0.0f, -0.0f, -0.0f, -0.0f};
        for (uint32_t m = tp.carriers; m != 0u; m &= m - 1u) {
            const uint32_t j = (uint32_t)__builtin_ctz(m);
            float tv[4];
            gfb_values<TABLE>(ps, tp, j, first, tab_s, tv);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = acc[e] + tv[e] * gcont_param(ps.g, sm[e], d, 2u * j + 1u); // A_j = a_j: a carrier
        }
        if (heard > 1u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = acc[e] / heard_f;
        }
        if (first + 4u <= ps.g.count) {
            *reinterpret_cast<float4 *>(ps.g.out + first) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e)
                if (first + e < ps.g.count) ps.g.out[first + e] = acc[e];
        }
    }
}

// ---- the chain, serial form: grid (feedback operators of the level), one wavefront each ----
__device__ inline uint4 gfb_load_words(const uint32_t *buf, uint32_t first, uint32_t count)
{
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (first + 4u <= count) {
        q = *reinterpret_cast<const uint4 *>(buf + first);
    } else {
        if (first < count) q.x = buf[first];
        if (first + 1u < count) q.y = buf[first + 1u];
        if (first + 2u < count) q.z = buf[first + 2u];
    }
    return q;
}
template <bool TABLE> __global__ __launch_bounds__(64) void k_gfb_chain_serial(GraphFbPass ps, uint32_t shapes, uint32_t chain_ops)
{
    __shared__ float tab_s[TABLE ? kWavetableSize : 4];
    __shared__ uint32_t phi_s[kSerialBlock];
    __shared__ float t_s[kSerialBlock];
    const uint32_t j = chain_ops >> (3u * blockIdx.x) & 7u, w = shapes >> (3u * j) & 7u, lane = threadIdx.x;
    if (TABLE && gfb_reads_table(w)) { // (per workgroup: SQUARE and SAW never read it)
        for (uint32_t i = lane; i < kWavetableSize / 4u; i += 64u)
            reinterpret_cast<float4 *>(tab_s)[i] = reinterpret_cast<const float4 *>(ps.g.wavetable)[i];
    }
    const uint32_t *phi = ps.g.words + (size_t)j * ps.g.lay.stride;
    float *t = gfb_tbuf(ps, j), *hist = gfb_hist(ps, j);
    const uint32_t count = ps.g.count;
    const float scaled = ps.scaled[j];
    float h1 = hist[0], h2 = hist[1];
    uint4 next = gfb_load_words(phi, 4u * lane, count);
    for (uint32_t base = 0; base < count; base += kSerialBlock) {
        phi_s[4u * lane] = next.x, phi_s[4u * lane + 1u] = next.y, phi_s[4u * lane + 2u] = next.z, phi_s[4u * lane + 3u] = next.w;
        __syncthreads();
        if (base + kSerialBlock < count) next = gfb_load_words(phi, base + kSerialBlock + 4u * lane, count); // in flight under the chain
        const uint32_t len = count - base < kSerialBlock ? count - base : kSerialBlock;
        if (lane == 0) {
            for (uint32_t n = 0; n < len; ++n) {
                const float v = gfb_step<TABLE>(w, phi_s[n], scaled, h1, h2, tab_s);
                t_s[n] = v;
                h2 = h1, h1 = v;
            }
        }
        __syncthreads();
        const uint32_t first = base + 4u * lane;
        if (first + 4u <= count) {
            *reinterpret_cast<float4 *>(t + first) = make_float4(t_s[4u * lane], t_s[4u * lane + 1u], t_s[4u * lane + 2u], t_s[4u * lane + 3u]);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e)
                if (first + e < count) t[first + e] = t_s[4u * lane + e];
        }
    }
    if (lane == 0) hist[0] = h1, hist[1] = h2;
}

// ---- the chain, relaxation form: grid (feedback operators of the level), one workgroup each, a lane per sample of a tile ----
template <bool TABLE> __global__ __launch_bounds__(kContThreads) void k_gfb_chain_relax(GraphFbPass ps, uint32_t shapes, uint32_t chain_ops)
{
    __shared__ float tab_s[TABLE ? kWavetableSize : 4];
    __shared__ float t_s[2][kRelaxTile];
    __shared__ uint32_t phi_s[kRelaxTile];
    __shared__ uint32_t flag_s[2][kContWaves];
    const uint32_t j = chain_ops >> (3u * blockIdx.x) & 7u, w = shapes >> (3u * j) & 7u, n = threadIdx.x;
    if (TABLE && gfb_reads_table(w)) cont_load_table(tab_s, ps.g.wavetable); // (the same branch for the whole workgroup)
    const uint32_t *phi = ps.g.words + (size_t)j * ps.g.lay.stride;
    float *t = gfb_tbuf(ps, j), *hist = gfb_hist(ps, j);
    const uint32_t count = ps.g.count, cap = ps.relax_cap;
    const float scaled = ps.scaled[j];
    float c1 = hist[0], c2 = hist[1]; // the carry into the tile: t of the two samples before it
    for (uint32_t base = 0; base < count; base += kRelaxTile) {
        const uint32_t len = count - base < kRelaxTile ? count - base : kRelaxTile;
        const bool live = n < len;
        const uint32_t p = live ? phi[base + n] : 0u;
        float mine = gfb_shape<TABLE>(w, p >> 17, tab_s); // the first guess: the feed-forward value
        phi_s[n] = p;
        t_s[0][n] = mine;
        __syncthreads();
        const uint32_t limit = cap < len ? cap : len; // after len sweeps every sample of the tile is final
        uint32_t cur = 0;
        bool settled = false;
        for (uint32_t s = 0; s < limit; ++s) {
            const float *src = t_s[cur];
            const float a = n >= 1u ? src[n - 1u] : c1;
            const float b = n >= 2u ? src[n - 2u] : (n == 1u ? c1 : c2);
            const float v = gfb_step<TABLE>(w, p, scaled, a, b, tab_s);
            const bool changed = live && __float_as_uint(v) != __float_as_uint(mine);
            t_s[cur ^ 1u][n] = v;
            mine = v;
            const bool wave_changed = __ballot(changed) != 0ull;
            if ((n & 63u) == 0u) flag_s[s & 1u][n >> 6] = wave_changed ? 1u : 0u;
            __syncthreads();
            cur ^= 1u;
            uint32_t any = 0;
#pragma unroll
            for (int q = 0; q < kContWaves; ++q) any |= flag_s[s & 1u][q];
            if (any == 0u) { // the same words for every lane: the whole workgroup leaves together
                settled = true;
                break;
            }
        }
        if (!settled && limit < len) { // the cap: samples 0 .. limit - 1 are final, the rest one after the other
            if (n == 0) {
                float *fin = t_s[cur];
                float h1 = fin[limit - 1u], h2 = limit >= 2u ? fin[limit - 2u] : c1;
                for (uint32_t i = limit; i < len; ++i) {
                    const float v = gfb_step<TABLE>(w, phi_s[i], scaled, h1, h2, tab_s);
                    fin[i] = v;
                    h2 = h1, h1 = v;
                }
            }
            __syncthreads();
        }
        const float *fin = t_s[cur];
        if (live) t[base + n] = fin[n];
        const float e1 = fin[len - 1u], e2 = len >= 2u ? fin[len - 2u] : c1;
        c1 = e1, c2 = e2;
        __syncthreads(); // the next tile writes t_s, phi_s and flag_s
    }
    if (n == 0) hist[0] = c1, hist[1] = c2;
}

template <bool TABLE>
hipError_t gfb_level(hipStream_t st, const GraphFbPass &ps, const GraphTopo &tp, uint32_t level_ops, uint32_t in_level, uint32_t first_slot,
                     uint32_t tiles, uint32_t num_cus)
{
    // With the 128 KiB table in LDS: one workgroup per compute unit, looping over its tiles; without it, two.
    const uint32_t resident = TABLE ? num_cus : 2u * num_cus;
    const uint32_t gx = tiles < resident ? tiles : resident;
    k_gfb_reduce<TABLE><<<dim3(gx, in_level), kContThreads, 0, st>>>(ps, tp, level_ops, tiles);
    if (hipError_t e = hipGetLastError()) return e;
    k_cont_scan<<<in_level, kContThreads, 0, st>>>(ps.g.words + ps.g.lay.totals, ps.g.words + ps.g.lay.carry + first_slot, tiles);
    if (hipError_t e = hipGetLastError()) return e;
    k_gfb_apply<TABLE><<<dim3(gx, in_level), kContThreads, 0, st>>>(ps, tp, level_ops, tiles);
    return hipGetLastError();
}

// the chains of the operators in `set` (a bit mask, all of one level), serially or as relaxations
hipError_t gfb_chains(hipStream_t st, const GraphFbPass &ps, const GraphTopo &tp, const uint32_t codes[8], uint32_t set, bool relax)
{
    uint32_t chain_ops = 0, in_launch = 0;
    bool table = false;
    for (uint32_t m = set; m != 0u; m &= m - 1u) {
        const uint32_t j = (uint32_t)__builtin_ctz(m);
        chain_ops |= j << (3u * in_launch++);
        table = table || waveform_reads_table(codes[j]);
    }
    if (in_launch == 0) return hipSuccess;
    if (relax) {
        if (table) k_gfb_chain_relax<true><<<in_launch, kContThreads, 0, st>>>(ps, tp.shapes, chain_ops);
        else k_gfb_chain_relax<false><<<in_launch, kContThreads, 0, st>>>(ps, tp.shapes, chain_ops);
    } else {
        if (table) k_gfb_chain_serial<true><<<in_launch, 64, 0, st>>>(ps, tp.shapes, chain_ops);
        else k_gfb_chain_serial<false><<<in_launch, 64, 0, st>>>(ps, tp.shapes, chain_ops);
    }
    return hipGetLastError();
}

} // namespace

hipError_t launch_graph_feedback_pass(hipStream_t st, const sots_voice_graph &graph, const uint32_t waveforms[8], const GraphFbPass &ps,
                                      uint32_t num_cus)
{
    if (ps.fb_mask == 0u) return launch_graph_continuous_pass(st, graph, waveforms, ps.g, num_cus); // no chain: 4.16's launches
    const GraphContPass &g = ps.g;
    if (!g.values || !g.wavetable || !g.words || !g.out || g.num_rows == 0 || g.hop == 0 || g.hop > 2u * g.half_n) return hipErrorInvalidValue;
    if (voice_graph_check(&graph)) return hipErrorInvalidValue;
    if (g.count == 0) return hipSuccess;
    const uint32_t ops = graph.num_operators, flagged = (uint32_t)__builtin_popcount(ps.fb_mask);
    // what the kernels' 32-bit indices and the scratch layout rest on
    if (ps.fb_mask >> ops) return hipErrorInvalidValue;
    if (g.count > graph_feedback_max_pass(ops, flagged) || g.count > g.lay.stride || (g.lay.stride & 3u) || (uint64_t)g.n0 + g.count > (1ull << 31))
        return hipErrorInvalidValue;
    const uint32_t tiles = (g.count + kContTile - 1u) / kContTile;
    if (tiles > g.lay.tiles || tiles > (uint32_t)kContThreads || num_cus == 0) return hipErrorInvalidValue;
    if (g.lay.totals < (size_t)ops * g.lay.stride || g.lay.carry < g.lay.totals + (size_t)8u * g.lay.tiles) return hipErrorInvalidValue;
    if ((ps.tbuf & 3u) || ps.tbuf < g.lay.carry + 8u || ps.hist < ps.tbuf + (size_t)flagged * g.lay.stride) return hipErrorInvalidValue;
    if (ps.relax_cap < 1u || ps.relax_cap > kRelaxCapMax) return hipErrorInvalidValue;
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
        uint32_t level_ops = 0, level_mask = 0;
        bool table = false; // some operator of the level has an unflagged modulator whose shape reads the table
        for (uint32_t s = 0; s < in_level; ++s) {
            const uint32_t j = lv.ops[lv.first[l] + s];
            level_ops |= j << (3u * s);
            level_mask |= 1u << j;
            for (uint32_t i = 0; i < j; ++i)
                table = table || ((graph.modulators[j] >> i & 1u) && !(ps.fb_mask >> i & 1u) && waveform_reads_table(codes[i]));
        }
        hipError_t e = table ? gfb_level<true>(st, ps, tp, level_ops, in_level, lv.first[l], tiles, num_cus)
                             : gfb_level<false>(st, ps, tp, level_ops, in_level, lv.first[l], tiles, num_cus);
        if (e != hipSuccess) return e;
        const uint32_t chains = level_mask & ps.fb_mask;
        e = gfb_chains(st, ps, tp, codes, chains & ~ps.forms, false);
        if (e != hipSuccess) return e;
        e = gfb_chains(st, ps, tp, codes, chains & ps.forms, true);
        if (e != hipSuccess) return e;
    }
    bool table = false;
    for (uint32_t j = 0; j < ops; ++j) table = table || ((graph.carriers >> j & 1u) && !(ps.fb_mask >> j & 1u) && waveform_reads_table(codes[j]));
    const uint32_t resident = table ? num_cus : 2u * num_cus, gx = tiles < resident ? tiles : resident;
    if (table) k_gfb_mix<true><<<gx, kContThreads, 0, st>>>(ps, tp, tiles);
    else k_gfb_mix<false><<<gx, kContThreads, 0, st>>>(ps, tp, tiles);
    return hipGetLastError();
}

} // namespace sots
