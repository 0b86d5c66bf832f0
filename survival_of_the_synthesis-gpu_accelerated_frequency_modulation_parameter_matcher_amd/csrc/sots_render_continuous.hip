// sots_render_continuous.hip -- phase-continuous rendering of a parameter track (sots_render_continuous):
// the track as ONE voice whose oscillators never restart.
//
// The phases are 32-bit words, unsigned 15.17 fixed point: the wrap of the wavetable is the wrap of the word, and an
// operator's phase is the EXCLUSIVE PREFIX SUM of its increments.  Integer addition is associative, so the sum is the same
// bits however it is tiled: a tile's increments are summed (reduce), the tile totals are scanned by one workgroup on top
// of the carry of the pass before (scan), and every tile scans its increments again on top of its base (apply) - three
// plain launches per operator stage in stream order.  No workgroup waits for another: no look-back, no flags, no grid
// barrier.  An operator's increment at sample n reads the phase of the operator before it at n, so the stages of a series
// voice follow each other through a phase buffer of one word per sample; the last stage writes the samples.
// The increments are made twice (reduce and apply) and not stored in between: a stored increment is 8 bytes of traffic per
// sample and stage, making it again is one table read from LDS and a dozen fp32 operations.
// Every fp32 expression is the CPU oracle's, uncontracted; tests/_render_continuous_model.py states the whole in NumPy.
#include "sots_render.h"
#include "sots_render_scan.h" // cont_fix, cont_load_table, cont_wave_scan, cont_block_scan, k_cont_scan

#pragma clang fp contract(off)

namespace sots {

namespace {

template <int KIND> struct ContVoice;
template <> struct ContVoice<SOTS_SYNTH_2OP> { static constexpr int OPS = 2, J = 1, D = 4; };
template <> struct ContVoice<SOTS_SYNTH_3OP_SERIES> { static constexpr int OPS = 3, J = 1, D = 6; };
template <> struct ContVoice<SOTS_SYNTH_TRIPLE_PAR> { static constexpr int OPS = 2, J = 3, D = 12; };
template <> struct ContVoice<SOTS_SYNTH_4OP_SERIES> { static constexpr int OPS = 4, J = 1, D = 8; };

// The parameters of sample n: the genes of its row (HOLD) or of its two rows (GLIDE), scaled as the synthesis kernels scale.
template <int KIND> struct ContParams {
    const float *a, *b;
    float t;
    bool lerp;
    const SynthParams *sp;
    __device__ ContParams(const ContPass &ps, uint32_t n)
    {
        constexpr int D = ContVoice<KIND>::D;
        uint32_t k, r;
        cont_position(n, ps.half_n, ps.hop, ps.num_rows, k, r);
        lerp = ps.glide && r != 0u;
        if (!ps.glide) k += 2u * r >= ps.hop ? 1u : 0u;
        a = ps.values + (size_t)(k - ps.row_base) * D;
        b = a + (lerp ? D : 0);
        t = lerp ? (float)r / (float)ps.hop : 0.0f;
        sp = &ps.sp;
    }
    __device__ float operator()(int i) const
    {
        const int sc = KIND == SOTS_SYNTH_TRIPLE_PAR ? (i & 3) : i; // the triple voice scales all three chains by entries 0..3
        float g = a[i];
        if (lerp) g = g + t * (b[i] - g);
        return sp->pmin[sc] + g * (sp->pmax[sc] - sp->pmin[sc]);
    }
};

// The increment of operator STAGE of chain j at sample n; prev is the phase word of operator STAGE - 1 at n (before its
// update, as the oracle reads it).  sots_oracle.c:130-215.
template <int KIND, int STAGE>
__device__ inline uint32_t cont_increment(const ContPass &ps, int j, uint32_t n, uint32_t prev, const float *tab)
{
    constexpr bool SERIES = KIND == SOTS_SYNTH_3OP_SERIES || KIND == SOTS_SYNTH_4OP_SERIES;
    const float c = (float)kWavetableSize / (float)SOTS_SAMPLE_RATE;
    const ContParams<KIND> p(ps, n);
    if constexpr (STAGE == 0) {
        return cont_fix(c * p(SERIES ? 1 : 4 * j));
    } else {
        float mul, off;
        if constexpr (SERIES) mul = p(2 * (STAGE - 1)) * p(2 * (STAGE - 1) + 1), off = p(2 * (STAGE - 1) + 3);
        else mul = p(4 * j) * p(4 * j + 1), off = p(4 * j + 2);
        const float cur = tab[prev >> 17] * mul + off;
        return cont_fix(c * cur);
    }
}

// the factor of the last operator's table value
template <int KIND> __device__ inline float cont_gain(const ContPass &ps, int j, uint32_t n)
{
    constexpr bool SERIES = KIND == SOTS_SYNTH_3OP_SERIES || KIND == SOTS_SYNTH_4OP_SERIES;
    constexpr int OPS = ContVoice<KIND>::OPS;
    const ContParams<KIND> p(ps, n);
    if constexpr (SERIES) return p(2 * (OPS - 1)) * p(2 * (OPS - 1) + 1);
    else return p(4 * j + 3);
}

// The four increments of this lane's quad of tile `tile` (0 behind the pass's end).  first: the quad's first pass sample.
template <int KIND, int STAGE>
__device__ inline void cont_quad(const ContPass &ps, int j, uint32_t first, const uint32_t *prev_buf, const float *tab, uint32_t inc[4])
{
    uint32_t prev[4] = {0u, 0u, 0u, 0u};
    if constexpr (STAGE > 0) {
        if (first + 4u <= ps.count) {
            const uint4 q = *reinterpret_cast<const uint4 *>(prev_buf + first);
            prev[0] = q.x, prev[1] = q.y, prev[2] = q.z, prev[3] = q.w;
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e)
                if (first + e < ps.count) prev[e] = prev_buf[first + e];
        }
    }
#pragma unroll
    for (uint32_t e = 0; e < 4u; ++e) inc[e] = first + e < ps.count ? cont_increment<KIND, STAGE>(ps, j, ps.n0 + first + e, prev[e], tab) : 0u;
}

// grid (tiles by stride, chains)
template <int KIND, int STAGE> __global__ __launch_bounds__(kContThreads) void k_cont_reduce(ContPass ps, uint32_t tiles)
{
    __shared__ float tab_s[STAGE > 0 ? kWavetableSize : 4];
    __shared__ uint32_t wtot[2][kContWaves];
    if constexpr (STAGE > 0) cont_load_table(tab_s, ps.wavetable);
    const int j = (int)blockIdx.y;
    const uint32_t *prev_buf = ps.words + ps.lay.phi[(STAGE + 1) & 1] + (size_t)j * ps.lay.stride;
    uint32_t *totals = ps.words + ps.lay.totals + (size_t)j * tiles;
    uint32_t parity = 0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x, parity ^= 1u) {
        uint32_t inc[4];
        cont_quad<KIND, STAGE>(ps, j, tile * kContTile + 4u * threadIdx.x, prev_buf, tab_s, inc);
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

// Not the last stage, grid (tiles by stride, chains): the stage's phase words.  The last stage, grid (tiles by stride): the
// chains one after the other in the workgroup, their products added in the reference's order, the output samples.
template <int KIND, int STAGE> __global__ __launch_bounds__(kContThreads) void k_cont_apply(ContPass ps, uint32_t tiles)
{
    constexpr bool LAST = STAGE == ContVoice<KIND>::OPS - 1;
    constexpr int J = ContVoice<KIND>::J;
    __shared__ float tab_s[STAGE > 0 ? kWavetableSize : 4];
    __shared__ uint32_t wtot[2][kContWaves];
    if constexpr (STAGE > 0) cont_load_table(tab_s, ps.wavetable);
    uint32_t parity = 0;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t first = tile * kContTile + 4u * threadIdx.x;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f}; // the last stage: tot[0] + tot[1] + tot[2], left to right
#pragma unroll
        for (int jj = 0; jj < (LAST ? J : 1); ++jj, parity ^= 1u) {
            const int j = LAST ? jj : (int)blockIdx.y;
            const uint32_t *prev_buf = ps.words + ps.lay.phi[(STAGE + 1) & 1] + (size_t)j * ps.lay.stride;
            uint32_t inc[4], total;
            cont_quad<KIND, STAGE>(ps, j, first, prev_buf, tab_s, inc);
            uint32_t phi = ps.words[ps.lay.totals + (size_t)j * tiles + tile] +
                           cont_block_scan(inc[0] + inc[1] + inc[2] + inc[3], wtot[parity], total);
            uint32_t w[4];
#pragma unroll
            for (uint32_t e = 0; e < 4u; ++e) w[e] = phi, phi += inc[e];
            if constexpr (!LAST) {
                uint32_t *dst = ps.words + ps.lay.phi[STAGE & 1] + (size_t)j * ps.lay.stride + first;
                if (first + 4u <= ps.count) {
                    *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
                } else {
#pragma unroll
                    for (uint32_t e = 0; e < 4u; ++e)
                        if (first + e < ps.count) dst[e] = w[e];
                }
            } else {
#pragma unroll
                for (uint32_t e = 0; e < 4u; ++e) {
                    const float x = first + e < ps.count ? tab_s[w[e] >> 17] * cont_gain<KIND>(ps, j, ps.n0 + first + e) : 0.0f;
                    acc[e] = jj == 0 ? x : acc[e] + x;
                }
            }
        }
        if constexpr (LAST) {
            if constexpr (J == 3) {
#pragma unroll
                for (uint32_t e = 0; e < 4u; ++e) acc[e] = acc[e] / 3.0f; // == (float)(double(sum) / 3.0), as the synthesis kernels state it
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
}

template <int KIND, int STAGE> hipError_t cont_stages_from(hipStream_t st, const ContPass &ps, uint32_t tiles, uint32_t num_cus)
{
    constexpr int OPS = ContVoice<KIND>::OPS, J = ContVoice<KIND>::J;
    constexpr bool LAST = STAGE == OPS - 1;
    // The table stages hold the 128 KiB wavetable in LDS: one workgroup per compute unit, looping over its tiles.
    const uint32_t resident = STAGE > 0 ? num_cus : 2u * num_cus;
    const uint32_t gx = tiles < resident ? tiles : resident;
    k_cont_reduce<KIND, STAGE><<<dim3(gx, J), kContThreads, 0, st>>>(ps, tiles);
    if (hipError_t e = hipGetLastError()) return e;
    k_cont_scan<<<J, kContThreads, 0, st>>>(ps.words + ps.lay.totals, ps.words + ps.lay.carry + STAGE * kContMaxChains, tiles);
    if (hipError_t e = hipGetLastError()) return e;
    k_cont_apply<KIND, STAGE><<<dim3(gx, LAST ? 1 : J), kContThreads, 0, st>>>(ps, tiles);
    if (hipError_t e = hipGetLastError()) return e;
    if constexpr (!LAST) return cont_stages_from<KIND, STAGE + 1>(st, ps, tiles, num_cus);
    else return hipSuccess;
}

} // namespace

hipError_t launch_continuous_pass(hipStream_t st, uint32_t kind, const ContPass &ps, uint32_t num_cus)
{
    if (!ps.values || !ps.wavetable || !ps.words || !ps.out || ps.num_rows == 0 || ps.hop == 0 || ps.hop > 2u * ps.half_n) return hipErrorInvalidValue;
    if (ps.count == 0) return hipSuccess;
    // what the kernels' 32-bit indices and the scratch layout rest on
    if (ps.count > kContMaxPass || ps.count > ps.lay.stride || (uint64_t)ps.n0 + ps.count > (1ull << 31)) return hipErrorInvalidValue;
    const uint32_t tiles = (ps.count + kContTile - 1u) / kContTile;
    if (tiles > ps.lay.tiles || num_cus == 0) return hipErrorInvalidValue;
    switch (kind) {
    case SOTS_SYNTH_2OP: return cont_stages_from<SOTS_SYNTH_2OP, 0>(st, ps, tiles, num_cus);
    case SOTS_SYNTH_3OP_SERIES: return cont_stages_from<SOTS_SYNTH_3OP_SERIES, 0>(st, ps, tiles, num_cus);
    case SOTS_SYNTH_TRIPLE_PAR: return cont_stages_from<SOTS_SYNTH_TRIPLE_PAR, 0>(st, ps, tiles, num_cus);
    case SOTS_SYNTH_4OP_SERIES: return cont_stages_from<SOTS_SYNTH_4OP_SERIES, 0>(st, ps, tiles, num_cus);
    default: return hipErrorInvalidValue;
    }
}

} // namespace sots
