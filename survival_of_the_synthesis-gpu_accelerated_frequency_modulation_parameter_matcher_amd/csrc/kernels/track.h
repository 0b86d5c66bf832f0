// track.h -- the run record: k_track (best-ever individual, per-generation history by pairwise tree sums), k_track_clear.
#pragma once
#include "common.h"

// contraction: off (the translation unit's default: the sums of the history add in a fixed tree, nothing multiplies and adds)
#pragma clang fp contract(off)
namespace sots { namespace {

// ------------------------------------------------------------------------------------
// run record (sots_track): best-ever individual and per-generation history, one workgroup per chunk, right after a
// generation's sortPopulation.  Reads rows 0..numParents-1 of the sorted half only - every sort mode and both selection
// plans place those each generation - and writes nothing the generation loop reads.
// ------------------------------------------------------------------------------------

// A context's 16384 parents are a quarter of a million floats for ONE workgroup: 1024 threads with sixteen loads in flight
// each keep that to a few memory round trips; a few dozen parents (chunks in flight) take four wavefronts.  The choice
// is a function of the row count and D alone, like everything else that shapes the sums.
constexpr uint32_t kTrackThreadsSmall = 256, kTrackThreadsLarge = 1024;
constexpr uint32_t kTrackLeaf = 16;   // rows a thread adds pairwise into one leaf of its tree
constexpr int kTrackLevels = 22;      // partial sums of a pairwise tree over up to 2^22 leaves per thread
inline uint32_t track_threads(uint32_t parents, uint32_t d) { return (uint64_t)parents * d > 8192u ? kTrackThreadsLarge : kTrackThreadsSmall; }

// Pairwise (tree) summation of a stream: level l holds the sum of a completed block of 2^l pushes; a push that finds its
// level taken adds the two blocks and carries the sum up, like a binary counter.  Every thread of the workgroup pushes
// the same number of times, so the tree's shape - and with it every rounding - depends on the row count alone.
struct TreeSum {
    float s[kTrackLevels];
    uint32_t n;
    __device__ __forceinline__ TreeSum() : n(0)
    {
#pragma unroll
        for (int l = 0; l < kTrackLevels; ++l) s[l] = 0.0f;
    }
    __device__ __forceinline__ void push(float v)
    {
        const uint32_t c = n++;
        bool open = true;
#pragma unroll
        for (int l = 0; l < kTrackLevels; ++l) {
            const bool taken = (c >> l) & 1u;
            const float up = s[l] + v;
            if (open && !taken) s[l] = v;
            if (open && taken) v = up;
            open = open && taken;
        }
    }
    // the blocks left over, smallest first
    __device__ __forceinline__ float total() const
    {
        float acc = 0.0f;
        bool has = false;
#pragma unroll
        for (int l = 0; l < kTrackLevels; ++l)
            if ((n >> l) & 1u) {
                acc = has ? s[l] + acc : s[l];
                has = true;
            }
        return acc;
    }
};

// the tree sum of x[(lane + k * lanes) * stride], k = 0, 1, ... while the row is below n: leaves of kTrackLeaf rows, added
// pairwise; rows past the end count as 0.0f (exact).  `groups` is the same for every thread.
__device__ __forceinline__ float track_column_sum(const float *__restrict__ x, uint32_t lane, uint32_t lanes, uint32_t stride,
                                                  uint32_t n, uint32_t groups, bool active)
{
    auto leaf = [&](uint32_t g) {
        float a[kTrackLeaf];
#pragma unroll
        for (uint32_t j = 0; j < kTrackLeaf; ++j) {
            const uint64_t r = (uint64_t)lane + (uint64_t)(g * kTrackLeaf + j) * lanes;
            a[j] = active && r < n ? x[r * stride] : 0.0f;
        }
#pragma unroll
        for (uint32_t w = kTrackLeaf / 2; w > 0; w >>= 1)
#pragma unroll
            for (uint32_t j = 0; j < w; ++j) a[j] = a[j] + a[j + w];
        return a[0];
    };
    if (groups == 1) return leaf(0); // (a tree of one leaf: what the cascade below returns, without running it)
    TreeSum sum;
    for (uint32_t g = 0; g < groups; ++g) sum.push(leaf(g));
    return sum.total();
}

// one wavefront joins the `count` (<= 1024) per-thread sums of a column: sixteen strided entries per lane pairwise, then
// a shuffle tree over the lanes.  Lane 0 holds the sum.
__device__ __forceinline__ float track_join(const float *col, uint32_t count, uint32_t lane)
{
    float a[16];
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) a[k] = lane + 64u * k < count ? col[lane + 64u * k] : 0.0f;
#pragma unroll
    for (uint32_t w = 8; w > 0; w >>= 1)
#pragma unroll
        for (uint32_t j = 0; j < w; ++j) a[j] = a[j] + a[j + w];
    float v = a[0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}

// meta[c] = {best-ever fitness bits, best-ever generation}; rows[c] = {values[16], steps[16]}; hist: [chunks][capacity]
// records of kTrackRecordFloats words (sots_gen_record).  slot == kTrackNoSlot: no history record this generation.
// blockDim.x = track_threads(parents, d).
__global__ __launch_bounds__(kTrackThreadsLarge) void k_track(const float *__restrict__ values, const float *__restrict__ steps,
                                                              const float *__restrict__ fitness, uint32_t p, uint32_t d, uint32_t parents,
                                                              uint32_t generation, uint32_t *__restrict__ meta, float *__restrict__ rows,
                                                              float *__restrict__ hist, uint32_t capacity, uint32_t slot)
{
    __shared__ float sm_fit[kTrackThreadsLarge];
    __shared__ float sm_step[kTrackThreadsLarge];
    const uint32_t c = blockIdx.x, t = threadIdx.x, threads = blockDim.x;
    const float *v = values + (size_t)c * p * d, *s = steps + (size_t)c * p * d, *f = fitness + (size_t)c * p;
    uint32_t *m = meta + 2u * (size_t)c;
    float *row = rows + (size_t)kTrackRowFloats * c;

    // best-ever: strictly better only, so a tie keeps the older record and NaN never wins
    const float f0 = f[0], worst = f[parents - 1];
    const float old = __uint_as_float(m[0]);
    const bool wins = f0 < old;
    const float best_ever = wins ? f0 : old;
    const bool record = slot != kTrackNoSlot;
    const uint32_t lanes = threads / d; // step sizes: thread t sums gene t % d over rows t / d, t / d + lanes, ...
    if (record) {
        // parent fitness: a strided tree sum per thread; step sizes: consecutive threads read consecutive floats
        const uint32_t per_f = (parents + threads - 1) / threads, per_s = (parents + lanes - 1) / lanes;
        sm_fit[t] = track_column_sum(f, t, threads, 1, parents, (per_f + kTrackLeaf - 1) / kTrackLeaf, true);
        const bool active = t < lanes * d;
        const uint32_t col = t % d, lane = t / d;
        const float sum = track_column_sum(s + col, lane, lanes, d, parents, (per_s + kTrackLeaf - 1) / kTrackLeaf, active);
        if (active) sm_step[col * lanes + lane] = sum;
    }
    __syncthreads(); // every thread holds the old record's fitness before thread 0 replaces it; the sums are in LDS
    if (wins) {
        if (t < d) row[t] = v[t];
        else if (t >= SOTS_MAX_DIMS && t < SOTS_MAX_DIMS + d) row[t] = s[t - SOTS_MAX_DIMS];
        if (t == 0) {
            m[0] = __float_as_uint(f0);
            m[1] = generation;
        }
    }
    if (!record) return;

    float *rec = hist + ((size_t)c * capacity + slot) * kTrackRecordFloats;
    const float count = (float)parents;
    const uint32_t wave = t / 64u, waves = threads / 64u, lane = t % 64u;
    // column d is the fitness; a wavefront joins the columns it is dealt
    for (uint32_t col = wave; col <= d; col += waves) {
        const float total = col < d ? track_join(sm_step + col * lanes, lanes, lane) : track_join(sm_fit, threads, lane);
        if (lane == 0) rec[col < d ? 8 + col : 4] = total / count;
    }
    if (t == 0) {
        reinterpret_cast<uint32_t *>(rec)[0] = generation;
        rec[1] = f0;
        rec[2] = best_ever;
        rec[3] = worst;
        rec[5] = 0.0f;
        rec[6] = 0.0f;
        rec[7] = 0.0f;
    }
    if (t >= d && t < SOTS_MAX_DIMS) rec[8 + t] = 0.0f;
}

// a cleared slot: fitness +inf, generation 0, zeroed rows
__global__ __launch_bounds__(256) void k_track_clear(uint32_t *__restrict__ meta, float *__restrict__ rows, uint32_t chunks)
{
    const uint32_t total = chunks * (2u + kTrackRowFloats);
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        if (e < 2u * chunks) meta[e] = e & 1u ? 0u : 0x7F800000u;
        else rows[e - 2u * chunks] = 0.0f;
    }
}

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
