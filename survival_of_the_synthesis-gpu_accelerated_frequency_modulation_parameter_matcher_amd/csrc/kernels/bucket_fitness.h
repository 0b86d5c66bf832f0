// bucket_fitness.h -- k_bucket_fitness: files the keys of a fitness array under their buckets (bkt_visit, sel_keys.h) where
// no spectral kernel has done so.  The kernel stood outside the unit's anonymous namespace, as a static function, and
// stays so: the namespace is part of a kernel's name and the name is part of the code object.
#pragma once
#include "common.h"
#include "sel_keys.h"

// contraction: off (the translation unit's default: keys are compared, nothing multiplies and adds)
#pragma clang fp contract(off)
namespace sots {

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

} // namespace sots

#pragma clang fp contract(off)
