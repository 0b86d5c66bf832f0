// sots_render_graph.hip -- phase-continuous rendering of a parameter track of the operator-graph voice, with or without
// feedback operators (sots_render_graph_continuous, sots_render_graph_feedback): the track as ONE voice
// whose oscillators never restart, for any feed-forward graph of 2 to 8 operators.
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
//
// Feedback never touches a phase: every Phi_j is still the exclusive prefix sum of its increments.  What an operator with
// beta_j != 0 adds is ONE chain over the samples, which turns its finished phase words and the constant B_j into its shaped
// values t_j(n) = shape(w_j, (Phi_j(n) + fix(B_j (t_j(n-1) + t_j(n-2)) / 2)) >> 17):
//   * after a level's reduce / scan / apply, one chain launch with the level's feedback operators in the grid reads Phi_j of
//     the pass and writes a float buffer t_j of the pass; only feedback operators have such a buffer;
//   * reduce, apply and mix take the value of a flagged modulator or carrier from its t buffer, decided by a scalar mask
//     argument (wavefront-uniform), and make every other operator's from its phase word.  With an empty mask there is no
//     chain launch and neither a t buffer nor hist is touched: that is the voice without feedback, whose launches take the
//     three kernels compiled without the test of the mask (FB false), the one body's second instantiation;
//   * between passes an operator carries its end phase and h1, h2.
// The chain has two forms with the same bits.  Serial: one wavefront per operator; the phase words come a block at a time by
// coalesced loads, the next block in flight while lane 0 runs the chain over the current one out of LDS, and t leaves a block
// at a time.  Relaxation: one workgroup per operator walks tiles of 1024 samples in order; a tile starts from the
// feed-forward values, every sweep recomputes every sample from its two predecessors in the other copy, and the tile is done
// at a sweep that changed no lane's bits - it then satisfies the recurrence everywhere, and the recurrence has one solution.
// Sweep k makes at least the first k samples final, so after relax_cap sweeps lane 0 finishes the tile from sample relax_cap.
// No workgroup waits for another, no atomics, no scratch.  Every fp32 expression is the definition's (include/sots_hip.h),
// uncontracted; tests/_render_graph_continuous_model.py and tests/_render_graph_feedback_model.py state the whole in NumPy.
//
// A voice whose feedback indices are genes (sots_render_graph_genes; GraphGenes, sots_render.h): a gene
// operator's B is a value per sample, made from the gene columns of the pass's rows like a frequency or a level.  Neither the
// scans nor the chain's exactness use the constancy of B.  Reduce, apply and mix are the kernels of every graph voice, fed the
// rows' first 2 OPS floats; only the chains are kernels of the voice's own (.._genes).  tests/_render_graph_genes_model.py
// states it.
#include <type_traits>

#include "sots_render.h"
#include "sots_render_scan.h" // cont_fix, cont_load_table, cont_block_scan, k_cont_scan
#include "sots_rules.h"       // graph_levels, graph_level_reads_table, waveform_reads_table, graph_feedback_max_pass

#pragma clang fp contract(off)

namespace sots {

namespace {

constexpr uint32_t kRelaxTile = 1024;  // samples per tile of the relaxation: one per lane
constexpr uint32_t kSerialBlock = 256; // phase words per block of the serial form: a quad per lane of one wavefront
static_assert(kRelaxTile == (uint32_t)kContThreads, "a relaxation tile is one sample per lane");

struct GraphTopo {
    uint32_t ops, carriers, shapes; // shapes: the codes, 3 bits per operator
    uint32_t modulators[8];
};

// Where sample n of the rendering takes its genes: row `a` (HOLD) or rows `a` and a + D at t between them (GLIDE)
struct GraphSample {
    const float *a;
    float t;
    bool lerp;
};
// (rows: the pass's rows, d floats each, from row_base on)
__device__ inline GraphSample graph_sample(const GraphPass &ps, const float *rows, uint32_t d, uint32_t n)
{
    uint32_t k, r;
    cont_position(n, ps.half_n, ps.hop, ps.num_rows, k, r);
    GraphSample s;
    s.lerp = ps.glide && r != 0u;
    if (!ps.glide) k += 2u * r >= ps.hop ? 1u : 0u;
    s.a = rows + (size_t)(k - ps.row_base) * d;
    s.t = s.lerp ? (float)r / (float)ps.hop : 0.0f;
    return s;
}
__device__ inline GraphSample graph_sample(const GraphPass &ps, uint32_t d, uint32_t n) { return graph_sample(ps, ps.values, d, n); }
// parameter g of the sample, scaled as the graph voice scales it: no folding of the ranges
__device__ inline float graph_param(const GraphPass &ps, const GraphSample &s, uint32_t d, uint32_t g)
{
    float v = s.a[g];
    if (s.lerp) v = v + s.t * (s.a[g + d] - v);
    return ps.sp.pmin[g] + v * (ps.sp.pmax[g] - ps.sp.pmin[g]);
}
// The rows of this lane's quad.  A sample behind the pass's end takes the pass's last sample's: rows that are on the device.
__device__ inline void graph_samples(const GraphPass &ps, uint32_t d, uint32_t first, GraphSample sm[4])
{
#pragma unroll
    for (uint32_t e = 0; e < 4u; ++e) {
        const uint32_t at = first + e < ps.count ? first + e : ps.count - 1u;
        sm[e] = graph_sample(ps, d, ps.n0 + at);
    }
}

// shape(w, i) of four indices, every case decided on the integer index (include/sots_hip.h).  w is wavefront-uniform.
// Without the table (TABLE false) the host has seen to it that w is SQUARE or SAW.
template <bool TABLE> __device__ inline void graph_shape(uint32_t w, const uint32_t at[4], const float *tab, float tv[4])
{
    constexpr uint32_t H = kWavetableSize / 2u, Q = kWavetableSize / 4u, M = kWavetableSize - 1u;
    if (w == SOTS_WAVE_SAW) {
#pragma unroll
        for (int e = 0; e < 4; ++e) tv[e] = (float)at[e] * 0x1p-14f - 1.0f;
        return;
    }
    if (!TABLE || w == SOTS_WAVE_SQUARE) {
#pragma unroll
        for (int e = 0; e < 4; ++e) tv[e] = at[e] < H ? 1.0f : -1.0f;
        return;
    }
    if constexpr (TABLE) {
        switch (w) {
        case SOTS_WAVE_HALF:
#pragma unroll
            for (int e = 0; e < 4; ++e) tv[e] = at[e] < H ? tab[at[e]] : 0.0f;
            break;
        case SOTS_WAVE_ABS:
#pragma unroll
            for (int e = 0; e < 4; ++e) tv[e] = fabsf(tab[at[e]]);
            break;
        case SOTS_WAVE_PULSE:
#pragma unroll
            for (int e = 0; e < 4; ++e) tv[e] = (at[e] & Q) == 0u ? fabsf(tab[at[e]]) : 0.0f;
            break;
        case SOTS_WAVE_EVEN: // (the read stays inside the table whatever the index; the upper half is +0)
#pragma unroll
            for (int e = 0; e < 4; ++e) tv[e] = at[e] < H ? tab[(2u * at[e]) & M] : 0.0f;
            break;
        case SOTS_WAVE_ABS_EVEN:
#pragma unroll
            for (int e = 0; e < 4; ++e) tv[e] = at[e] < H ? fabsf(tab[(2u * at[e]) & M]) : 0.0f;
            break;
        default:
#pragma unroll
            for (int e = 0; e < 4; ++e) tv[e] = tab[at[e]];
            break;
        }
    }
}
// shape(w, i) of one index: graph_shape's own cases
template <bool TABLE> __device__ inline float graph_shape(uint32_t w, uint32_t at, const float *tab)
{
    const uint32_t a4[4] = {at, at, at, at};
    float tv[4];
    graph_shape<TABLE>(w, a4, tab, tv);
    return tv[0];
}
// t_j(n) from the phase word and the two shaped values before it
template <bool TABLE> __device__ inline float graph_step(uint32_t w, uint32_t phi, float scaled, float h1, float h2, const float *tab)
{
    const float g = (h1 + h2) * 0.5f;
    const uint32_t z = phi + cont_fix(scaled * g);
    return graph_shape<TABLE>(w, z >> 17, tab);
}

// the t buffer's position among the flagged operators, in ascending j
__device__ inline uint32_t graph_slot(uint32_t mask, uint32_t j) { return (uint32_t)__builtin_popcount(mask & ((1u << j) - 1u)); }
__device__ inline float *graph_tbuf(const GraphPass &ps, uint32_t j)
{
    return reinterpret_cast<float *>(ps.words + ps.lay.tbuf) + (size_t)graph_slot(ps.fb_mask, j) * ps.lay.stride;
}
__device__ inline float *graph_hist(const GraphPass &ps, uint32_t j)
{
    return reinterpret_cast<float *>(ps.words + ps.lay.hist) + 2u * graph_slot(ps.fb_mask, j);
}

// four words of a buffer of the pass at `first` (a multiple of 4), 0 behind the pass's end
__device__ inline uint4 graph_load_words(const uint32_t *buf, uint32_t first, uint32_t count)
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

// this lane's quad of operator i's shaped values: from its t buffer where i is flagged (0 behind the pass's end), else made
// from its phase words.  FB false: the host has seen to it that no operator is flagged, and the kernels are compiled without
// the test - with it the renderings without feedback were 1.5 to 2 % slower on dense8
template <bool TABLE, bool FB>
__device__ inline void graph_values(const GraphPass &ps, const GraphTopo &tp, uint32_t i, uint32_t first, const float *tab, float tv[4])
{
    if (FB && (ps.fb_mask >> i & 1u)) { // a kernel argument: wavefront-uniform
        const uint4 q = graph_load_words(reinterpret_cast<const uint32_t *>(graph_tbuf(ps, i)), first, ps.count);
        tv[0] = __uint_as_float(q.x), tv[1] = __uint_as_float(q.y), tv[2] = __uint_as_float(q.z), tv[3] = __uint_as_float(q.w);
        return;
    }
    const uint4 q = graph_load_words(ps.words + (size_t)i * ps.lay.stride, first, ps.count);
    const uint32_t at[4] = {q.x >> 17, q.y >> 17, q.z >> 17, q.w >> 17};
    graph_shape<TABLE>(tp.shapes >> (3u * i) & 7u, at, tab, tv);
}

// The four increments of operator j in this lane's quad (0 behind the pass's end).  first: the quad's first pass sample.
template <bool TABLE, bool FB>
__device__ inline void graph_quad(const GraphPass &ps, const GraphTopo &tp, uint32_t j, uint32_t first, const float *tab, uint32_t inc[4])
{
    const float c = (float)kWavetableSize / (float)SOTS_SAMPLE_RATE;
    const uint32_t d = 2u * tp.ops;
    GraphSample sm[4];
    graph_samples(ps, d, first, sm);
    float cur[4] = {-0.0f, -0.0f, -0.0f, -0.0f};
    const uint32_t mods = tp.modulators[j];
    for (uint32_t m = mods; m != 0u; m &= m - 1u) { // set bits in ascending i: wavefront-uniform
        const uint32_t i = (uint32_t)__builtin_ctz(m);
        float tv[4];
        graph_values<TABLE, FB>(ps, tp, i, first, tab, tv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float level = graph_param(ps, sm[e], d, 2u * i) * graph_param(ps, sm[e], d, 2u * i + 1u); // A_i = f_i a_i: a modulator
            cur[e] = cur[e] + tv[e] * level;
        }
    }
#pragma unroll
    for (uint32_t e = 0; e < 4u; ++e) {
        const float f = graph_param(ps, sm[e], d, 2u * j);
        const float x = mods != 0u ? cur[e] + f : f;
        inc[e] = first + e < ps.count ? cont_fix(c * x) : 0u;
    }
}

// grid (tiles by stride, operators of the level); level_ops: the level's operators, 3 bits each, in grid.y order
template <bool TABLE, bool FB> __global__ __launch_bounds__(kContThreads) void k_graph_reduce(GraphPass ps, GraphTopo tp, uint32_t level_ops, uint32_t tiles)
{
    __shared__ float tab_s[TABLE ? kWavetableSize : 4];
    __shared__ uint32_t wtot[2][kContWaves];
    if constexpr (TABLE) cont_load_table(tab_s, ps.wavetable);
    const uint32_t j = level_ops >> (3u * blockIdx.y) & 7u;
    uint32_t *totals = ps.words + ps.lay.totals + (size_t)blockIdx.y * tiles;
    uint32_t parity = 0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, parity ^= 1u) {
        uint32_t inc[4];
        graph_quad<TABLE, FB>(ps, tp, j, tile * kContTile + 4u * threadIdx.x, tab_s, inc);
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
template <bool TABLE, bool FB> __global__ __launch_bounds__(kContThreads) void k_graph_apply(GraphPass ps, GraphTopo tp, uint32_t level_ops, uint32_t tiles)
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
        graph_quad<TABLE, FB>(ps, tp, j, first, tab_s, inc);
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
template <bool TABLE, bool FB> __global__ __launch_bounds__(kContThreads) void k_graph_mix(GraphPass ps, GraphTopo tp, uint32_t tiles)
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
        graph_samples(ps, d, first, sm);
        float acc[4] = {-0.0f, -0.0f, -0.0f, -0.0f};
        for (uint32_t m = tp.carriers; m != 0u; m &= m - 1u) {
            const uint32_t j = (uint32_t)__builtin_ctz(m);
            float tv[4];
            graph_values<TABLE, FB>(ps, tp, j, first, tab_s, tv);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = acc[e] + tv[e] * graph_param(ps, sm[e], d, 2u * j + 1u); // A_j = a_j: a carrier
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

// ---- the chain, serial form: grid (feedback operators of the level), one wavefront each ----
template <bool TABLE> __global__ __launch_bounds__(64) void k_graph_chain_serial(GraphPass ps, uint32_t shapes, uint32_t chain_ops)
{
    __shared__ float tab_s[TABLE ? kWavetableSize : 4];
    __shared__ uint32_t phi_s[kSerialBlock];
    __shared__ float t_s[kSerialBlock];
    const uint32_t j = chain_ops >> (3u * blockIdx.x) & 7u, w = shapes >> (3u * j) & 7u, lane = threadIdx.x;
    if (TABLE && waveform_reads_table(w)) { // (per workgroup: SQUARE and SAW never read it)
        for (uint32_t i = lane; i < kWavetableSize / 4u; i += 64u)
            reinterpret_cast<float4 *>(tab_s)[i] = reinterpret_cast<const float4 *>(ps.wavetable)[i];
    }
    const uint32_t *phi = ps.words + (size_t)j * ps.lay.stride;
    float *t = graph_tbuf(ps, j), *hist = graph_hist(ps, j);
    const uint32_t count = ps.count;
    const float scaled = ps.scaled[j];
    float h1 = hist[0], h2 = hist[1];
    uint4 next = graph_load_words(phi, 4u * lane, count);
    for (uint32_t base = 0; base < count; base += kSerialBlock) {
        phi_s[4u * lane] = next.x, phi_s[4u * lane + 1u] = next.y, phi_s[4u * lane + 2u] = next.z, phi_s[4u * lane + 3u] = next.w;
        __syncthreads();
        if (base + kSerialBlock < count) next = graph_load_words(phi, base + kSerialBlock + 4u * lane, count); // in flight under the chain
        const uint32_t len = count - base < kSerialBlock ? count - base : kSerialBlock;
        if (lane == 0) {
            for (uint32_t n = 0; n < len; ++n) {
                const float v = graph_step<TABLE>(w, phi_s[n], scaled, h1, h2, tab_s);
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
template <bool TABLE> __global__ __launch_bounds__(kContThreads) void k_graph_chain_relax(GraphPass ps, uint32_t shapes, uint32_t chain_ops)
{
    __shared__ float tab_s[TABLE ? kWavetableSize : 4];
    __shared__ float t_s[2][kRelaxTile];
    __shared__ uint32_t phi_s[kRelaxTile];
    __shared__ uint32_t flag_s[2][kContWaves];
    const uint32_t j = chain_ops >> (3u * blockIdx.x) & 7u, w = shapes >> (3u * j) & 7u, n = threadIdx.x;
    if (TABLE && waveform_reads_table(w)) cont_load_table(tab_s, ps.wavetable); // (the same branch for the whole workgroup)
    const uint32_t *phi = ps.words + (size_t)j * ps.lay.stride;
    float *t = graph_tbuf(ps, j), *hist = graph_hist(ps, j);
    const uint32_t count = ps.count, cap = ps.relax_cap;
    const float scaled = ps.scaled[j];
    float c1 = hist[0], c2 = hist[1]; // the carry into the tile: t of the two samples before it
    for (uint32_t base = 0; base < count; base += kRelaxTile) {
        const uint32_t len = count - base < kRelaxTile ? count - base : kRelaxTile;
        const bool live = n < len;
        const uint32_t p = live ? phi[base + n] : 0u;
        float mine = graph_shape<TABLE>(w, p >> 17, tab_s); // the first guess: the feed-forward value
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
            const float v = graph_step<TABLE>(w, p, scaled, a, b, tab_s);
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
                    const float v = graph_step<TABLE>(w, phi_s[i], scaled, h1, h2, tab_s);
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

// ---- the chains of a voice whose feedback indices are genes ----
// The two forms above with B a value per sample.  They are kernels of their own, their text beside the forms' above and not
// shared with it: a body that both call compiles the kernels above to other code (the same instructions in another order),
// and a voice without gene operators is to launch what it launched before, byte for byte (tools/codeobj_diff.py).
// An operator of gn.mask (a kernel argument: the branch is wavefront-uniform) takes B per sample from the gene columns of the
// pass's rows, made by all lanes outside the chain and kept in a register and in LDS; the other operators of the launch keep
// their constant.  No global access inside a chain.

// B of gene operator j at pass sample `at`: the gene of the sample's rows, held or glided and scaled as any gene, made
// effective, times K - one fp32 product.  A sample behind the pass's end takes the pass's last sample's rows.
__device__ inline float graph_gene_scaled(const GraphPass &ps, const GraphGenes &gn, uint32_t j, uint32_t at)
{
    const uint32_t q = gn.column[j];
    const GraphSample s = graph_sample(ps, gn.rows, gn.count, ps.n0 + (at < ps.count ? at : ps.count - 1u));
    float v = s.a[q - gn.first];
    if (s.lerp) v = v + s.t * (s.a[q - gn.first + gn.count] - v);
    return effective_feedback(ps.sp.pmin[q] + v * (ps.sp.pmax[q] - ps.sp.pmin[q])) * kFeedbackScale;
}

// serial form: k_graph_chain_serial with the block's 256 values of B, four per lane, in LDS beside the phase words
template <bool TABLE> __global__ __launch_bounds__(64) void k_graph_chain_serial_genes(GraphPass ps, GraphGenes gn, uint32_t shapes, uint32_t chain_ops)
{
    __shared__ float tab_s[TABLE ? kWavetableSize : 4];
    __shared__ uint32_t phi_s[kSerialBlock];
    __shared__ float big_s[kSerialBlock];
    __shared__ float t_s[kSerialBlock];
    const uint32_t j = chain_ops >> (3u * blockIdx.x) & 7u, w = shapes >> (3u * j) & 7u, lane = threadIdx.x;
    if (TABLE && waveform_reads_table(w)) {
        for (uint32_t i = lane; i < kWavetableSize / 4u; i += 64u)
            reinterpret_cast<float4 *>(tab_s)[i] = reinterpret_cast<const float4 *>(ps.wavetable)[i];
    }
    const uint32_t *phi = ps.words + (size_t)j * ps.lay.stride;
    float *t = graph_tbuf(ps, j), *hist = graph_hist(ps, j);
    const uint32_t count = ps.count;
    const bool gene = gn.mask >> j & 1u;
    const float scaled = ps.scaled[j];
    float h1 = hist[0], h2 = hist[1];
    uint4 next = graph_load_words(phi, 4u * lane, count);
    for (uint32_t base = 0; base < count; base += kSerialBlock) {
        phi_s[4u * lane] = next.x, phi_s[4u * lane + 1u] = next.y, phi_s[4u * lane + 2u] = next.z, phi_s[4u * lane + 3u] = next.w;
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e) big_s[4u * lane + e] = gene ? graph_gene_scaled(ps, gn, j, base + 4u * lane + e) : scaled;
        __syncthreads();
        if (base + kSerialBlock < count) next = graph_load_words(phi, base + kSerialBlock + 4u * lane, count); // in flight under the chain
        const uint32_t len = count - base < kSerialBlock ? count - base : kSerialBlock;
        if (lane == 0) {
            for (uint32_t n = 0; n < len; ++n) {
                const float v = graph_step<TABLE>(w, phi_s[n], big_s[n], h1, h2, tab_s);
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

// relaxation: k_graph_chain_relax with this lane's sample's B made once per tile, before the sweeps, and kept in a register;
// the in-order finish reads it from LDS
template <bool TABLE>
__global__ __launch_bounds__(kContThreads) void k_graph_chain_relax_genes(GraphPass ps, GraphGenes gn, uint32_t shapes, uint32_t chain_ops)
{
    __shared__ float tab_s[TABLE ? kWavetableSize : 4];
    __shared__ float t_s[2][kRelaxTile];
    __shared__ uint32_t phi_s[kRelaxTile];
    __shared__ float big_s[kRelaxTile];
    __shared__ uint32_t flag_s[2][kContWaves];
    const uint32_t j = chain_ops >> (3u * blockIdx.x) & 7u, w = shapes >> (3u * j) & 7u, n = threadIdx.x;
    if (TABLE && waveform_reads_table(w)) cont_load_table(tab_s, ps.wavetable);
    const uint32_t *phi = ps.words + (size_t)j * ps.lay.stride;
    float *t = graph_tbuf(ps, j), *hist = graph_hist(ps, j);
    const uint32_t count = ps.count, cap = ps.relax_cap;
    const bool gene = gn.mask >> j & 1u;
    float c1 = hist[0], c2 = hist[1];
    for (uint32_t base = 0; base < count; base += kRelaxTile) {
        const uint32_t len = count - base < kRelaxTile ? count - base : kRelaxTile;
        const bool live = n < len;
        const uint32_t p = live ? phi[base + n] : 0u;
        const float scaled = gene ? graph_gene_scaled(ps, gn, j, base + n) : ps.scaled[j];
        float mine = graph_shape<TABLE>(w, p >> 17, tab_s);
        phi_s[n] = p;
        big_s[n] = scaled;
        t_s[0][n] = mine;
        __syncthreads();
        const uint32_t limit = cap < len ? cap : len;
        uint32_t cur = 0;
        bool settled = false;
        for (uint32_t s = 0; s < limit; ++s) {
            const float *src = t_s[cur];
            const float a = n >= 1u ? src[n - 1u] : c1;
            const float b = n >= 2u ? src[n - 2u] : (n == 1u ? c1 : c2);
            const float v = graph_step<TABLE>(w, p, scaled, a, b, tab_s);
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
            if (any == 0u) {
                settled = true;
                break;
            }
        }
        if (!settled && limit < len) {
            if (n == 0) {
                float *fin = t_s[cur];
                float h1 = fin[limit - 1u], h2 = limit >= 2u ? fin[limit - 2u] : c1;
                for (uint32_t i = limit; i < len; ++i) {
                    const float v = graph_step<TABLE>(w, phi_s[i], big_s[i], h1, h2, tab_s);
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
        __syncthreads(); // the next tile writes t_s, phi_s, big_s and flag_s
    }
    if (n == 0) hist[0] = c1, hist[1] = c2;
}

// f(TABLE, FB) with the two decided at run time as compile-time constants
template <class F> hipError_t graph_pick(bool table, bool fb, F f)
{
    using Yes = std::true_type;
    using No = std::false_type;
    return table ? (fb ? f(Yes{}, Yes{}) : f(Yes{}, No{})) : (fb ? f(No{}, Yes{}) : f(No{}, No{}));
}

template <bool TABLE, bool FB>
hipError_t graph_level(hipStream_t st, const GraphPass &ps, const GraphTopo &tp, uint32_t level_ops, uint32_t in_level, uint32_t first_slot,
                       uint32_t tiles, uint32_t num_cus)
{
    // With the 128 KiB table in LDS: one workgroup per compute unit, looping over its tiles; without it, two.
    const uint32_t resident = TABLE ? num_cus : 2u * num_cus;
    const uint32_t gx = tiles < resident ? tiles : resident;
    k_graph_reduce<TABLE, FB><<<dim3(gx, in_level), kContThreads, 0, st>>>(ps, tp, level_ops, tiles);
    if (hipError_t e = hipGetLastError()) return e;
    k_cont_scan<<<in_level, kContThreads, 0, st>>>(ps.words + ps.lay.totals, ps.words + ps.lay.carry + first_slot, tiles);
    if (hipError_t e = hipGetLastError()) return e;
    k_graph_apply<TABLE, FB><<<dim3(gx, in_level), kContThreads, 0, st>>>(ps, tp, level_ops, tiles);
    return hipGetLastError();
}

// the chains of the operators in `set` (a bit mask, all of one level), serially or as relaxations
// (gn: null for a voice without gene operators)
hipError_t graph_chains(hipStream_t st, const GraphPass &ps, const GraphTopo &tp, const uint32_t codes[8], uint32_t set, bool relax,
                        const GraphGenes *gn)
{
    uint32_t chain_ops = 0, in_launch = 0;
    bool table = false;
    for (uint32_t m = set; m != 0u; m &= m - 1u) {
        const uint32_t j = (uint32_t)__builtin_ctz(m);
        chain_ops |= j << (3u * in_launch++);
        table = table || waveform_reads_table(codes[j]);
    }
    if (in_launch == 0) return hipSuccess;
    if (gn) {
        if (relax) {
            if (table) k_graph_chain_relax_genes<true><<<in_launch, kContThreads, 0, st>>>(ps, *gn, tp.shapes, chain_ops);
            else k_graph_chain_relax_genes<false><<<in_launch, kContThreads, 0, st>>>(ps, *gn, tp.shapes, chain_ops);
        } else {
            if (table) k_graph_chain_serial_genes<true><<<in_launch, 64, 0, st>>>(ps, *gn, tp.shapes, chain_ops);
            else k_graph_chain_serial_genes<false><<<in_launch, 64, 0, st>>>(ps, *gn, tp.shapes, chain_ops);
        }
    } else if (relax) {
        if (table) k_graph_chain_relax<true><<<in_launch, kContThreads, 0, st>>>(ps, tp.shapes, chain_ops);
        else k_graph_chain_relax<false><<<in_launch, kContThreads, 0, st>>>(ps, tp.shapes, chain_ops);
    } else {
        if (table) k_graph_chain_serial<true><<<in_launch, 64, 0, st>>>(ps, tp.shapes, chain_ops);
        else k_graph_chain_serial<false><<<in_launch, 64, 0, st>>>(ps, tp.shapes, chain_ops);
    }
    return hipGetLastError();
}

} // namespace

hipError_t launch_graph_pass(hipStream_t st, const sots_voice_graph &graph, const uint32_t waveforms[8], const GraphPass &ps, uint32_t num_cus,
                             const GraphGenes *genes)
{
    if (!ps.values || !ps.wavetable || !ps.words || !ps.out || ps.num_rows == 0 || ps.hop == 0 || ps.hop > 2u * ps.half_n) return hipErrorInvalidValue;
    if (voice_graph_check(&graph)) return hipErrorInvalidValue;
    if (ps.count == 0) return hipSuccess;
    const uint32_t ops = graph.num_operators, flagged = (uint32_t)__builtin_popcount(ps.fb_mask);
    const GraphLayout &lay = ps.lay;
    // what the kernels' 32-bit indices and the scratch layout rest on
    if (ps.fb_mask >> ops) return hipErrorInvalidValue;
    // a voice with gene operators: every one of them is flagged, and its column is the one the rules give it
    const GraphGenes *gn = genes && genes->mask ? genes : nullptr;
    if (gn) {
        if (!gn->rows || (gn->mask & ~ps.fb_mask) || gn->first != 2u * ops || gn->count != feedback_gene_count(gn->mask) ||
            gn->first + gn->count > SOTS_MAX_DIMS)
            return hipErrorInvalidValue;
        for (uint32_t j = 0; j < ops; ++j)
            if ((gn->mask >> j & 1u) && gn->column[j] != feedback_gene_column(ops, gn->mask, j)) return hipErrorInvalidValue;
    }
    if (ps.count > graph_feedback_max_pass(ops, flagged) || ps.count > lay.stride || (lay.stride & 3u) || (uint64_t)ps.n0 + ps.count > (1ull << 31))
        return hipErrorInvalidValue;
    const uint32_t tiles = (ps.count + kContTile - 1u) / kContTile;
    if (tiles > lay.tiles || tiles > (uint32_t)kContThreads || num_cus == 0) return hipErrorInvalidValue;
    if (lay.totals < (size_t)ops * lay.stride || lay.carry < lay.totals + (size_t)8u * lay.tiles) return hipErrorInvalidValue;
    if (flagged != 0u) {
        if (lay.hist < lay.carry + 8u || (lay.tbuf & 3u) || lay.tbuf < lay.hist + 16u) return hipErrorInvalidValue;
        if (ps.relax_cap < 1u || ps.relax_cap > kRelaxCapMax) return hipErrorInvalidValue;
    }
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
        for (uint32_t s = 0; s < in_level; ++s) {
            const uint32_t j = lv.ops[lv.first[l] + s];
            level_ops |= j << (3u * s);
            level_mask |= 1u << j;
        }
        hipError_t e = graph_pick(graph_level_reads_table(graph, lv, codes, l, ps.fb_mask), flagged != 0u, [&](auto table, auto fb) {
            return graph_level<decltype(table)::value, decltype(fb)::value>(st, ps, tp, level_ops, in_level, lv.first[l], tiles, num_cus);
        });
        if (e != hipSuccess) return e;
        const uint32_t chains = level_mask & ps.fb_mask;
        e = graph_chains(st, ps, tp, codes, chains & ~ps.forms, false, gn);
        if (e != hipSuccess) return e;
        e = graph_chains(st, ps, tp, codes, chains & ps.forms, true, gn);
        if (e != hipSuccess) return e;
    }
    bool table = false; // some carrier's value is made from its phase word by a shape that reads the table
    for (uint32_t j = 0; j < ops; ++j) table = table || ((graph.carriers >> j & 1u) && !(ps.fb_mask >> j & 1u) && waveform_reads_table(codes[j]));
    const uint32_t resident = table ? num_cus : 2u * num_cus, gx = tiles < resident ? tiles : resident;
    return graph_pick(table, flagged != 0u, [&](auto tb, auto fb) {
        k_graph_mix<decltype(tb)::value, decltype(fb)::value><<<gx, kContThreads, 0, st>>>(ps, tp, tiles);
        return hipGetLastError();
    });
}

} // namespace sots
