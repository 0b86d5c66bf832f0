// variation.h -- the Philox4x32-10 draws and the rule of variation (make_gene: recombine_source, mutate_gene), which every
// kernel that makes individuals calls; the variation kernels of a context, of the chunks in flight and of the chunk queue.
#pragma once
#include "common.h"

// contraction: off (the translation unit's default: recombination and the value half of mutation round as written)
#pragma clang fp contract(off)
namespace sots { namespace {

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

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
