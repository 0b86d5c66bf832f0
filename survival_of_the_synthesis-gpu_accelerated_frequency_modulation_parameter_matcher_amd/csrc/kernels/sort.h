// sort.h -- the full sortPopulation: the island exchange carried by every kernel that moves sorted rows (ex_*), the tile
// sort, the rank passes and the kernels that move the rows (k_sort_tiles ... k_sort_gather).
#pragma once
#include "common.h"

// contraction: off (the translation unit's default: keys are compared and rows are copied, every float as it is)
#pragma clang fp contract(off)
namespace sots { namespace {

// ------------------------------------------------------------------------------------
// sortPopulation, ocl_program.cl:664-711 (rank sort) / Population::bubbleSortPopulation,
// Evolutionary_Strategy.hpp:108-124.  Ascending by fitness, equal fitness keeps the lower
// original index first (the CPU's stable order), NaN after every number.  Implemented as a
// bitonic network over unique 64-bit keys (order-preserving fitness bits << 32 | index).
// ------------------------------------------------------------------------------------
// ---- island exchange inside the kernels that move the sorted rows (SortExchange, sots_kernels.h) -------------
// a destination row that belongs to an immigrant: the local row that sorted there is NOT written
__device__ __forceinline__ bool ex_immigrant_row(const SortExchange &ex, uint32_t dst)
{
    return ex.imm != nullptr && dst - ex.imm_first < ex.imm_rows;
}
// element `c` (0..d-1 values, d..2d-1 steps, 2d fitness) of destination row dst also goes to the packed elite rows
__device__ __forceinline__ void ex_sink(const SortExchange &ex, uint32_t dst, uint32_t c, uint32_t d, float v)
{
    if (dst < ex.sink_rows) ex.sink[(size_t)dst * (2 * d + 1) + (c == 2 * d ? 0u : c + 1u)] = v;
}
// the immigrant rows themselves (k_unpack_rows' copy), by the threads of ONE workgroup
__device__ __forceinline__ void ex_unpack(const SortExchange &ex, float *__restrict__ vout, float *__restrict__ sout,
                                          float *__restrict__ fout, uint32_t d, uint32_t tid, uint32_t threads)
{
    if (ex.imm == nullptr) return;
    const uint32_t w = 2 * d + 1, total = ex.imm_rows * w;
    for (uint32_t e = tid; e < total; e += threads) {
        const uint32_t r = e / w, c = e - r * w, dst = ex.imm_first + r;
        const uint32_t sr = r < ex.skip_first ? r : r + ex.skip_count;
        const float v = ex.imm[(size_t)sr * w + c]; // packed rows: [fitness, values.., steps..]
        if (c == 0) fout[dst] = v;
        else if (c <= d) vout[(size_t)dst * d + (c - 1)] = v;
        else sout[(size_t)dst * d + (c - 1 - d)] = v;
        if (dst < ex.sink_rows) ex.sink[(size_t)dst * w + c] = v;
    }
}

constexpr int kSortThreads = 1024;
constexpr uint32_t kSortTile = 4096; // keys per LDS tile (32 KiB)
constexpr uint32_t kSortSmall = 1024; // populations sorted by one workgroup in one launch (k_sort_small)

__device__ __forceinline__ uint64_t make_key(float f, uint32_t idx)
{
    uint32_t u;
    if (f != f) {
        u = 0xFFFFFFFFu;
    } else {
        u = __float_as_uint(f == 0.0f ? 0.0f : f);
        u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    return ((uint64_t)u << 32) | idx;
}

// Padding slot g >= P of the power-of-two key array: after every real key (NaN included) and
// unique, which the counting merges rely on.
__device__ __forceinline__ uint64_t pad_key(uint32_t g) { return 0xFFFFFFFF00000000ull | g; }

__device__ __forceinline__ void cmp_swap(uint64_t &a, uint64_t &b, bool ascending)
{
    if ((a > b) == ascending) {
        const uint64_t t = a;
        a = b;
        b = t;
    }
}

// Builds the keys of one tile and sorts it completely (all steps with k <= tile).
__global__ __launch_bounds__(kSortThreads) void k_sort_tiles(const float *__restrict__ fitness,
                                                             uint64_t *__restrict__ keys, uint32_t p_len,
                                                             uint32_t tile, uint32_t alternate)
{
    __shared__ uint64_t s[kSortTile];
    const uint32_t base = blockIdx.x * tile;
    // alternate != 0: odd tiles end up descending, ready for further global bitonic merges;
    // alternate == 0: every tile ascending (rank merge)
    const uint32_t dir_base = alternate ? base : 0u;
    for (uint32_t i = threadIdx.x; i < tile; i += blockDim.x) {
        const uint32_t g = base + i;
        s[i] = g < p_len ? make_key(fitness[g], g) : pad_key(g);
    }
    __syncthreads();
    for (uint32_t k = 2; k <= tile; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < tile / 2; t += blockDim.x) {
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const uint32_t hi = lo | j;
                const bool asc = (((dir_base + lo) & k) == 0);
                uint64_t a = s[lo], b = s[hi];
                cmp_swap(a, b, asc);
                s[lo] = a;
                s[hi] = b;
            }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < tile; i += blockDim.x) keys[base + i] = s[i];
}

// 1024-key tile for the rank merge, without workgroup barriers in the sorting network: each
// of the four wavefronts bitonic-sorts its own run of 256 keys in its private quarter of the
// LDS buffer (the LDS operations of one wavefront execute in order, so the 36 steps need no
// s_barrier), then every key's place in the tile is its index in its own run plus its lower
// bound in the other three runs (24 LDS reads), the same counting argument as the tile merge.
constexpr uint32_t kRunKeys = 256;

__global__ __launch_bounds__(256) void k_sort_tiles_1k(const float *__restrict__ fitness,
                                                       uint64_t *__restrict__ keys, uint32_t p_len)
{
    __shared__ uint64_t runs[4 * kRunKeys];
    __shared__ uint64_t merged[4 * kRunKeys];
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t base = blockIdx.x * 4 * kRunKeys + wave * kRunKeys;
    uint64_t *__restrict__ run = runs + wave * kRunKeys;
#pragma unroll
    for (uint32_t r = 0; r < kRunKeys / kWave; ++r) {
        const uint32_t i = lane + kWave * r, g = base + i;
        run[i] = g < p_len ? make_key(fitness[g], g) : pad_key(g);
    }
    for (uint32_t k = 2; k <= kRunKeys; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            __builtin_amdgcn_wave_barrier();
            asm volatile("" ::: "memory");
#pragma unroll
            for (uint32_t r = 0; r < kRunKeys / 2 / kWave; ++r) {
                const uint32_t t = lane + kWave * r;
                const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const uint32_t hi = lo | j;
                uint64_t a = run[lo], b = run[hi];
                cmp_swap(a, b, (lo & k) == 0);
                run[lo] = a;
                run[hi] = b;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kRunKeys / kWave; ++r) {
        const uint32_t i = lane + kWave * r;
        const uint64_t x = run[i];
        uint32_t rank = i;
#pragma unroll
        for (uint32_t o = 1; o < 4; ++o) {
            const uint64_t *__restrict__ other = runs + ((wave + o) & 3u) * kRunKeys;
            uint32_t pos = 0;
#pragma unroll
            for (uint32_t step = kRunKeys >> 1; step >= 1; step >>= 1) pos += (other[pos + step - 1] < x) ? step : 0u;
            rank += pos + ((other[pos] < x) ? 1u : 0u);
        }
        merged[rank] = x;
    }
    __syncthreads();
    uint64_t *__restrict__ out = keys + (size_t)blockIdx.x * 4 * kRunKeys;
    for (uint32_t i = threadIdx.x; i < 4 * kRunKeys; i += 256) out[i] = merged[i];
}

// One compare-exchange step (k, j) with j >= tile, over the whole padded array.
__global__ __launch_bounds__(256) void k_sort_global_step(uint64_t *__restrict__ keys, uint32_t n_pad,
                                                          uint32_t k, uint32_t j)
{
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_pad / 2; t += gridDim.x * blockDim.x) {
        const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const uint32_t hi = lo | j;
        const bool asc = ((lo & k) == 0);
        uint64_t a = keys[lo], b = keys[hi];
        cmp_swap(a, b, asc);
        keys[lo] = a;
        keys[hi] = b;
    }
}

// The remaining steps j = tile/2 .. 1 of merge size k, tile-local.
__global__ __launch_bounds__(kSortThreads) void k_sort_tile_merge(uint64_t *__restrict__ keys, uint32_t k,
                                                                  uint32_t tile)
{
    __shared__ uint64_t s[kSortTile];
    const uint32_t base = blockIdx.x * tile;
    for (uint32_t i = threadIdx.x; i < tile; i += blockDim.x) s[i] = keys[base + i];
    __syncthreads();
    const bool asc = ((base & k) == 0); // k > tile: the direction is uniform over the tile
    for (uint32_t j = tile >> 1; j > 0; j >>= 1) {
        for (uint32_t t = threadIdx.x; t < tile / 2; t += blockDim.x) {
            const uint32_t lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
            const uint32_t hi = lo | j;
            uint64_t a = s[lo], b = s[hi];
            cmp_swap(a, b, asc);
            s[lo] = a;
            s[hi] = b;
        }
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < tile; i += blockDim.x) keys[base + i] = s[i];
}

// ---- rank merge of sorted tiles ------------------------------------------------------
// With T sorted tiles of unique keys, the final position of a key is the number of keys
// below it = its index in its own tile + sum over the other tiles of lower_bound(tile, key).
// Workgroup (a, b) stages tile b in LDS and binary-searches every key of tile a in it;
// the T partial counts per key are then summed by the scatter kernel, which moves the
// (2D+1)-float row straight to its final place.  Two launches instead of the ~15 of the
// global bitonic steps, and every CU is busy.
constexpr int kRankThreads = 256;
constexpr uint32_t kRankGroup = 8;      // tiles staged in LDS per workgroup (tile = 1024: 64 KiB)
constexpr uint32_t kRankLdsKeys = 8192; // LDS capacity in keys

// Workgroup (a, g): keys of tile a against tiles [g*GROUP, (g+1)*GROUP); writes one partial
// count per key of a.  Keys are unique, so against its own tile a key's lower bound is its
// sorted index and no tile needs a special case.  The tiles are staged by LDS-DMA (all pieces
// in flight at once) and the GROUP x 4 binary searches of a thread advance together, one level
// per trip, so a trip has GROUP x 4 independent LDS reads in flight instead of 4.
// MERGE (large populations, first of two levels): the grid has one workgroup per tile, which ranks its
// keys inside its OWN group of GROUP tiles only and writes them to their place in the group's
// sorted run of GROUP * tile keys (merged[]); the second level then ranks runs instead of tiles.
template <uint32_t GROUP, bool MERGE = false>
__global__ __launch_bounds__(kRankThreads) void k_sort_rank_pairs(const uint64_t *__restrict__ keys,
                                                                  uint16_t *__restrict__ partial,
                                                                  uint32_t n_pad, uint32_t tile,
                                                                  uint64_t *__restrict__ merged = nullptr)
{
    __shared__ uint64_t s[kRankLdsKeys];
    const uint32_t a = blockIdx.x, g = MERGE ? blockIdx.x / GROUP : blockIdx.y;
    const uint64_t *__restrict__ kb = keys + (size_t)g * GROUP * tile;
    {
        typedef __attribute__((address_space(3))) void *lds_ptr_t;
        const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x & (kWave - 1);
        constexpr uint32_t kChunk = kWave * 2; // keys per wavefront instruction (16 B per lane)
        for (uint32_t ch = wave; ch < GROUP * tile / kChunk; ch += kRankThreads / kWave)
            __builtin_amdgcn_global_load_lds(kb + ch * kChunk + lane * 2u, (lds_ptr_t)(s + ch * kChunk), 16, 0, 0);
        __builtin_amdgcn_s_waitcnt(0); // the copies have landed
    }
    __syncthreads();
    const uint64_t *__restrict__ ka = keys + (size_t)a * tile;
    uint16_t *__restrict__ out = partial + (size_t)g * n_pad + (size_t)a * tile;
    for (uint32_t i0 = threadIdx.x; i0 < tile; i0 += 4 * kRankThreads) {
        uint64_t x[4];
        uint32_t pos[GROUP][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t i = i0 + q * kRankThreads;
            x[q] = i < tile ? ka[i] : 0ull;
#pragma unroll
            for (uint32_t bb = 0; bb < GROUP; ++bb) pos[bb][q] = 0;
        }
        for (uint32_t step = tile >> 1; step >= 1; step >>= 1) {
#pragma unroll
            for (uint32_t bb = 0; bb < GROUP; ++bb)
#pragma unroll
                for (int q = 0; q < 4; ++q) pos[bb][q] += (s[bb * tile + pos[bb][q] + step - 1] < x[q]) ? step : 0u;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t total = 0;
#pragma unroll
            for (uint32_t bb = 0; bb < GROUP; ++bb) total += pos[bb][q] + ((s[bb * tile + pos[bb][q]] < x[q]) ? 1u : 0u);
            const uint32_t i = i0 + q * kRankThreads;
            if constexpr (MERGE) {
                if (i < tile) merged[(size_t)g * GROUP * tile + total] = x[q];
            } else {
                if (i < tile) out[i] = (uint16_t)total;
            }
        }
    }
}

// 64 consecutive slots of the tile-sorted key array per workgroup: four quarter-sums of the
// partial counts per slot (all 256 lanes load), then the rows move to their final places.
__global__ __launch_bounds__(kRankThreads) void k_sort_rank_scatter(const uint64_t *__restrict__ keys,
                                                                    const uint16_t *__restrict__ partial,
                                                                    const float *__restrict__ vin,
                                                                    const float *__restrict__ sin,
                                                                    const float *__restrict__ fin,
                                                                    float *__restrict__ vout, float *__restrict__ sout,
                                                                    float *__restrict__ fout, uint32_t n_pad,
                                                                    uint32_t groups, uint32_t p_len, uint32_t d,
                                                                    uint32_t first_row, SortExchange ex)
{
    constexpr uint32_t kSlots = 64;
    if (blockIdx.x == 0) ex_unpack(ex, vout, sout, fout, d, threadIdx.x, kRankThreads);
    __shared__ uint32_t part[4][kSlots];
    __shared__ uint32_t src_row[kSlots];
    const uint32_t j = threadIdx.x & (kSlots - 1), quarter = threadIdx.x / kSlots;
    const uint32_t e = blockIdx.x * kSlots + j;
    uint32_t sum = 0;
    for (uint32_t g = quarter; g < groups; g += 4) sum += partial[(size_t)g * n_pad + e];
    part[quarter][j] = sum;
    if (quarter == 0) src_row[j] = (uint32_t)keys[e]; // >= P for padding keys
    __syncthreads();
    const uint32_t w = 2 * d + 1;
    for (uint32_t t = threadIdx.x; t < kSlots * w; t += kRankThreads) {
        const uint32_t jj = t / w, c = t - jj * w;
        const uint32_t src = src_row[jj];
        if (src >= p_len) continue;
        const uint32_t dst = part[0][jj] + part[1][jj] + part[2][jj] + part[3][jj];
        if (dst < first_row) continue; // rows the selection kernels have already placed
        if (ex_immigrant_row(ex, dst)) continue;
        const float v = c < d ? vin[(size_t)src * d + c] : c < 2 * d ? sin[(size_t)src * d + (c - d)] : fin[src];
        if (c < d) vout[(size_t)dst * d + c] = v;
        else if (c < 2 * d) sout[(size_t)dst * d + (c - d)] = v;
        else fout[dst] = v;
        ex_sink(ex, dst, c, d, v);
    }
}

// Row r of the new half <- row (keys[r] & 0xffffffff) of the old half.
__global__ __launch_bounds__(256) void k_sort_gather(const uint64_t *__restrict__ keys,
                                                     const float *__restrict__ vin,
                                                     const float *__restrict__ sin,
                                                     const float *__restrict__ fin, float *__restrict__ vout,
                                                     float *__restrict__ sout, float *__restrict__ fout,
                                                     uint32_t p_len, uint32_t d, uint32_t first_row, SortExchange ex)
{
    const uint32_t w = 2 * d + 1;
    const uint32_t total = p_len * w;
    if (blockIdx.x == 0) ex_unpack(ex, vout, sout, fout, d, threadIdx.x, blockDim.x);
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x + first_row * w; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t r = e / w, c = e - r * w;
        if (ex_immigrant_row(ex, r)) continue;
        const uint32_t src = (uint32_t)keys[r];
        const float v = c < d ? vin[(size_t)src * d + c] : c < 2 * d ? sin[(size_t)src * d + (c - d)] : fin[src];
        if (c < d) vout[(size_t)r * d + c] = v;
        else if (c < 2 * d) sout[(size_t)r * d + (c - d)] = v;
        else fout[r] = v;
        ex_sink(ex, r, c, d, v);
    }
}

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
