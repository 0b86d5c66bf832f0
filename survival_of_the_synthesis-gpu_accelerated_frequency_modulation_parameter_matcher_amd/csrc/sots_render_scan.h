// sots_render_scan.h -- what the two phase-continuous renderers share on the device (sots_render_continuous.hip, DESIGN.md
// 4.10; sots_render_graph_continuous.hip): fix(), the table in LDS, the scans of a wavefront and of a
// workgroup, and the kernel that scans a pass's tile totals.  Everything is in an anonymous namespace: each of the two files
// has its own copy, and nothing here is visible outside them.  Internal to libsots_hip.so.
#pragma once

#include "sots_render.h"

#pragma clang fp contract(off)

namespace sots {

namespace {

constexpr int kContThreads = 1024; // 16 wavefronts: a lane owns 4 consecutive samples of a tile
constexpr int kContWaves = kContThreads / 64;
static_assert(kContTile == 4u * kContThreads, "a tile is one quad per lane");

// fix(x): x in wavetable entries -> 15.17 fixed point, rint (ties to even), reduced mod 2^32; 0 where |x 2^17| < 2^62 fails (NaN too)
__device__ inline uint32_t cont_fix(float x)
{
    const float y = x * 131072.0f;
    return fabsf(y) < 0x1p62f ? (uint32_t)(long long)rintf(y) : 0u;
}

__device__ inline void cont_load_table(float *tab_s, const float *tab)
{
    for (uint32_t i = threadIdx.x; i < kWavetableSize / 4u; i += kContThreads)
        reinterpret_cast<float4 *>(tab_s)[i] = reinterpret_cast<const float4 *>(tab)[i];
    __syncthreads();
}

// inclusive sum over the wavefront's lanes
__device__ inline uint32_t cont_wave_scan(uint32_t x, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// Exclusive sum of one word per lane over the workgroup, and the workgroup's total.  wtot: kContWaves words that no lane
// still reads from the call before the last (the callers alternate between two).  One barrier.
__device__ inline uint32_t cont_block_scan(uint32_t v, uint32_t *wtot, uint32_t &total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t incl = cont_wave_scan(v, lane);
    if (lane == 63u) wtot[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)kContWaves; ++w) {
        const uint32_t x = wtot[w];
        before += w < wave ? x : 0u;
        all += x;
    }
    total = all;
    return before + incl - v;
}

// one workgroup per chain: totals -> bases (carry-in + exclusive prefix), carry-out.  A pass has at most one tile per lane.
static_assert(kContMaxPass / kContTile <= (uint32_t)kContThreads, "the tile totals of a pass are one word per lane");
__global__ __launch_bounds__(kContThreads) void k_cont_scan(uint32_t *totals_all, uint32_t *carry_all, uint32_t tiles)
{
    __shared__ uint32_t wtot[kContWaves];
    uint32_t *totals = totals_all + (size_t)blockIdx.x * tiles;
    const uint32_t carry = carry_all[blockIdx.x], i = threadIdx.x;
    uint32_t total;
    const uint32_t excl = cont_block_scan(i < tiles ? totals[i] : 0u, wtot, total);
    if (i < tiles) totals[i] = carry + excl;
    if (i == 0) carry_all[blockIdx.x] = carry + total;
}

} // namespace

} // namespace sots
