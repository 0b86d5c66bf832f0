// select_tiles.h -- the selection in two launches (k_sel_tiles, k_sel_merge4, k_sel_rank_scatter) and the single-workgroup
// sort that shares its register network (k_sort_small).
#pragma once
#include "common.h"
#include "sel_keys.h"
#include "sort.h"
#include "stamps.h"

// contraction: off (the translation unit's default: keys are compared and rows are copied, every float as it is)
#pragma clang fp contract(off)
namespace sots { namespace {

// ------------------------------------------------------------------------------------
// Selection for the fused generation loop: the best `need` rows IN ORDER and nothing else.
// The next recombination reads whole parent blocks only (recombine_source, variation.h;
// ocl_program.cl:99-112), so inside sots_execute_generations the order of the other rows is
// never looked at; the full order is produced (by launch_sort, from the untouched unsorted half)
// when somebody reads the population.  Rows 0..need-1 are bit-identical to the full sort's.
//
// Two launches.  k_sel_tiles sorts tiles of 1024 (fitness bits, index) keys: one key per lane,
// 16 wavefronts sort 64 keys each in registers (bitonic network over lane exchanges, no LDS
// traffic, no barrier), then every key's place in the tile is its lane plus its lower bound in
// the other 15 runs.  It writes the sorted fitness bits and indices as two u32 arrays and, per
// tile, the four keys at positions 255, 511, 767, 1023 ("samples").
// k_sel_rank_scatter (one workgroup per CU) finds v* = the ceil(need/256)-th smallest sample:
// at least need keys are <= v*, and every key <= v* lies in its tile's first
// 256 * (samples_t <= v*) + 256 positions.  Only those prefixes (need + 256 * tiles keys when
// there are no ties: 128 KiB at P = 65536) are staged in LDS as 4-byte fitness bits; a staged key's
// rank is the sum of its lower bounds in every staged prefix, and keys whose rank is below `need`
// move their rows.  Tiles are contiguous index ranges, so "equal fitness, lower index first" needs
// no index in LDS: against an EARLIER tile an equal key counts (<=), against a LATER one it does
// not (<).  Keys above v* get ranks >= need (every key <= v* is staged and there are >= need of
// them), so no check can fail and there is no fallback path; prefixes that exceed the LDS are staged
// in several passes.
// ------------------------------------------------------------------------------------
constexpr uint32_t kSelTile = 1024, kSelSamples = 4, kSelQuantum = kSelTile / kSelSamples;
constexpr uint32_t kSelThreads = 1024, kSelLanesPerKey = 8, kSelKeysPerRound = kSelThreads / kSelLanesPerKey;
constexpr uint32_t kSelCap = 35328;                 // staged keys per pass: 138 KiB of LDS
constexpr uint32_t kSelSkew = 4;                    // consecutive tiles start 4 more words (16 B) off the 1 KiB grid, see below
// the rank kernel handles 16..64 tiles of 1024 keys (P <= 65536) and, for P = 131072, 32 tiles of 4096 keys merged four by
// four (k_sel_merge4).  Same-box A/B of the un-instrumented loop (profiles/r03_experiments.md): at P = 131072 the selection
// beats the two-level full sort (237 against 244 us per generation), at 262144 it loses (496 against 482), so it stops at 128 tiles
constexpr uint32_t kSelMinTiles = 16, kSelMaxTiles = 128, kSelMaxOwn = 512; // kSelMaxTiles: tiles the rank kernel handles (of either size)


template <uint32_t K, uint32_t J>
__device__ __forceinline__ void bitonic_step(uint32_t &b, uint32_t &i, uint32_t lane)
{
    const uint32_t pb = lane_xor<J>(b), pi = lane_xor<J>(i);
    const bool keep_min = ((lane & J) == 0) == ((lane & K) == 0);
    const bool mine_less = b < pb || (b == pb && i < pi);
    if (keep_min != mine_less) {
        b = pb;
        i = pi;
    }
}
template <uint32_t K, uint32_t J>
__device__ __forceinline__ void bitonic_merge(uint32_t &b, uint32_t &i, uint32_t lane)
{
    bitonic_step<K, J>(b, i, lane);
    if constexpr (J > 1) bitonic_merge<K, J / 2>(b, i, lane);
}

// SPLIT workgroups per tile (blockIdx = tile + part * tiles): a tile is 16 wavefronts on ONE CU, and with the 64 tiles of
// P = 65536 three quarters of the GPU idle while each of those CUs answers 1440 wavefront-wide LDS reads of the searches.
// Every workgroup of a tile sorts all 16 runs (the searches need them; the register network is cheap), then only the
// wavefronts of ITS runs - a quarter, one per SIMD - search and write.
#ifndef SOTS_SEL_SPLIT
#define SOTS_SEL_SPLIT 4
#endif
template <uint32_t SPLIT>
__global__ __launch_bounds__(kSelTile) void k_sel_tiles(const float *__restrict__ fitness, uint32_t *__restrict__ kbits,
                                                         uint32_t *__restrict__ kidx, uint32_t *__restrict__ samples,
                                                         uint32_t p_len, uint32_t tiles)
{
    constexpr uint32_t kRuns = kSelTile / kWave;
    __shared__ uint32_t runs[kSelTile];
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const uint32_t tile = SPLIT == 1 ? blockIdx.x : blockIdx.x % tiles, part = SPLIT == 1 ? 0u : blockIdx.x / tiles;
    const uint32_t g = tile * kSelTile + tid;
    SOTS_PHASE_BEGIN();
    uint32_t b = g < p_len ? order_bits(fitness[g]) : kSelPadBits, i = g; // padding keys sort last, by index
#ifdef SOTS_STAMP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the stamp below then includes the fitness load
#endif
    SOTS_PHASE(8);
    bitonic_merge<2, 1>(b, i, lane);
    bitonic_merge<4, 2>(b, i, lane);
    bitonic_merge<8, 4>(b, i, lane);
    bitonic_merge<16, 8>(b, i, lane);
    bitonic_merge<32, 16>(b, i, lane);
    bitonic_merge<64, 32>(b, i, lane);
    runs[tid] = b;
    __syncthreads();
    SOTS_PHASE(9);
    if (SPLIT > 1 && wave / (kRuns / SPLIT) != part) return;
    // place in the tile = lane + lower bounds in the other 15 runs, all 15 searches advanced level by level so
    // that the LDS reads of a level are in flight together.  A run of an earlier wavefront holds lower indices,
    // so its equal keys come first (count <=, i.e. < b + 1), a later run's do not (<).
    uint32_t pos[kRuns], thr[kRuns]; // absolute positions in runs[]; "entries below thr" is what is counted
#pragma unroll
    for (uint32_t w = 0; w < kRuns; ++w) {
        pos[w] = w * kWave;
        thr[w] = w == wave ? 0u : b + (w < wave ? 1u : 0u); // own run: nothing counts (the lane is added below)
    }
#pragma unroll
    for (uint32_t step = kWave / 2; step >= 1; step >>= 1) {
#pragma unroll
        for (uint32_t w = 0; w < kRuns; ++w) pos[w] += runs[pos[w] + step - 1] < thr[w] ? step : 0u;
    }
    uint32_t rank = lane;
#pragma unroll
    for (uint32_t w = 0; w < kRuns; ++w) rank += pos[w] - w * kWave + (runs[pos[w]] < thr[w] ? 1u : 0u);
    SOTS_PHASE(10);
    const size_t o = (size_t)tile * kSelTile + rank;
    kbits[o] = b;
    kidx[o] = i;
    if ((rank & (kSelQuantum - 1)) == kSelQuantum - 1) {
        samples[tile * kSelSamples + rank / kSelQuantum] = b;
        samples[tiles * kSelSamples + tile * kSelSamples + rank / kSelQuantum] = i; // indices behind all the bits
    }
    SOTS_PHASE(11);
}

// A whole population of at most 1024 rows in ONE launch and one workgroup (the reference's default sizes are this
// small, and there a launch costs as much as the sort): k_sel_tiles' network - one key per lane, 64-key runs sorted in
// registers, a key's place = its lane + its lower bounds in the other runs - and then the workgroup moves the rows,
// a lane per output element.  Same order as the full sort: fitness, equal fitness by index, NaN last.
// SEG (chunks in flight): workgroup b sorts the b-th block of p_len rows, the grid one workgroup per chunk.
template <uint32_t RUNS, bool SEG = false>
__global__ __launch_bounds__(RUNS *kWave) void k_sort_small(const float *__restrict__ vin, const float *__restrict__ sin,
                                                            const float *__restrict__ fin, float *__restrict__ vout,
                                                            float *__restrict__ sout, float *__restrict__ fout,
                                                            uint32_t p_len, uint32_t d, uint32_t first_row, SortExchange ex)
{
    if constexpr (SEG) {
        const size_t rows = (size_t)blockIdx.x * p_len;
        vin += rows * d, sin += rows * d, fin += rows;
        vout += rows * d, sout += rows * d, fout += rows;
    }
    __shared__ uint32_t runs[RUNS * kWave], from[RUNS * kWave];
    ex_unpack(ex, vout, sout, fout, d, threadIdx.x, RUNS * kWave);
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    uint32_t b = tid < p_len ? order_bits(fin[tid]) : kSelPadBits, i = tid;
    bitonic_merge<2, 1>(b, i, lane);
    bitonic_merge<4, 2>(b, i, lane);
    bitonic_merge<8, 4>(b, i, lane);
    bitonic_merge<16, 8>(b, i, lane);
    bitonic_merge<32, 16>(b, i, lane);
    bitonic_merge<64, 32>(b, i, lane);
    uint32_t rank = lane;
    if constexpr (RUNS > 1) {
        runs[tid] = b;
        __syncthreads();
        uint32_t pos[RUNS], thr[RUNS];
#pragma unroll
        for (uint32_t w = 0; w < RUNS; ++w) {
            pos[w] = w * kWave;
            thr[w] = w == wave ? 0u : b + (w < wave ? 1u : 0u);
        }
#pragma unroll
        for (uint32_t step = kWave / 2; step >= 1; step >>= 1) {
#pragma unroll
            for (uint32_t w = 0; w < RUNS; ++w) pos[w] += runs[pos[w] + step - 1] < thr[w] ? step : 0u;
        }
#pragma unroll
        for (uint32_t w = 0; w < RUNS; ++w) rank += pos[w] - w * kWave + (runs[pos[w]] < thr[w] ? 1u : 0u);
    }
    // from[place] = the row that sorted there (padding keys sort behind every row).  The rows then move with lane =
    // OUTPUT element: a wavefront's stores are consecutive addresses and its loads runs of d consecutive floats - one
    // workgroup is one CU's address path, and a lane-per-row move (64 cache lines per instruction, 2 d + 1
    // instructions each way) took twice as long as the sort itself at d = 12.
    from[rank] = i;
    __syncthreads();
    constexpr uint32_t T = RUNS * kWave;
    if (tid < p_len && tid >= first_row && !ex_immigrant_row(ex, tid)) {
        const float f = fin[from[tid]];
        fout[tid] = f;
        ex_sink(ex, tid, 2 * d, d, f);
    }
    const uint32_t qd = T / d, rd = T - qd * d; // uniform: one scalar division per launch
    uint32_t r = tid / d, c = tid - r * d;
    while (r < p_len) { // four elements per trip, their loads in flight together
        uint32_t dst[4], row[4];
        float v[4], s[4];
        bool ok[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            row[q] = r, dst[q] = r * d + c;
            ok[q] = r < p_len && r >= first_row && !ex_immigrant_row(ex, r);
            if (ok[q]) {
                const uint32_t src = from[r] * d + c;
                v[q] = vin[src], s[q] = sin[src];
            }
            r += qd, c += rd;
            if (c >= d) c -= d, ++r;
        }
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q)
            if (ok[q]) {
                const uint32_t cq = dst[q] - row[q] * d;
                vout[dst[q]] = v[q], sout[dst[q]] = s[q];
                ex_sink(ex, row[q], cq, d, v[q]), ex_sink(ex, row[q], d + cq, d, s[q]);
            }
    }
}

// Four neighbouring sorted tiles of 1024 keys -> one sorted tile of 4096 with a sample every 512 keys.  For
// populations of 128 k and more the rank kernel's work (staged keys x tiles x search depth) is quartered by
// having a quarter of the tiles.  One workgroup per group of four: the 4096 fitness-bit words sit in LDS, a key's
// place = its position in its own tile + its lower bounds in the three siblings (earlier tile: <=, later: <).
constexpr uint32_t kSelBigTile = 4 * kSelTile, kSelBigQuantum = 512, kSelBigSamples = kSelBigTile / kSelBigQuantum;

__global__ __launch_bounds__(kSelTile) void k_sel_merge4(const uint32_t *__restrict__ kbits, const uint32_t *__restrict__ kidx,
                                                          uint32_t *__restrict__ obits, uint32_t *__restrict__ oidx,
                                                          uint32_t *__restrict__ samples)
{
    __shared__ uint32_t s[kSelBigTile];
    const uint32_t tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * kSelBigTile;
    uint32_t b[4], i[4];
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t) { // thread `tid` holds position `tid` of each of the four tiles
        b[t] = kbits[base + t * kSelTile + tid];
        i[t] = kidx[base + t * kSelTile + tid];
        s[t * kSelTile + tid] = b[t];
    }
    __syncthreads();
    uint32_t pos[4][4], thr[4][4]; // [own tile][sibling]: absolute search positions in s[]
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t)
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) {
            pos[t][u] = u * kSelTile;
            thr[t][u] = u == t ? 0u : b[t] + (u < t ? 1u : 0u); // bits <= 0xFFFFFFFE: no wrap
        }
#pragma unroll
    for (uint32_t step = kSelTile / 2; step >= 1; step >>= 1) {
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t)
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u)
                if (u != t) pos[t][u] += s[pos[t][u] + step - 1] < thr[t][u] ? step : 0u;
    }
    const uint32_t ns = gridDim.x * kSelBigSamples;
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t) {
        uint32_t rank = tid;
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u)
            if (u != t) rank += pos[t][u] - u * kSelTile + (s[pos[t][u]] < thr[t][u] ? 1u : 0u);
        obits[base + rank] = b[t];
        oidx[base + rank] = i[t];
        if ((rank & (kSelBigQuantum - 1)) == kSelBigQuantum - 1) {
            samples[blockIdx.x * kSelBigSamples + rank / kSelBigQuantum] = b[t];
            samples[ns + blockIdx.x * kSelBigSamples + rank / kSelBigQuantum] = i[t];
        }
    }
}

constexpr uint32_t kSelChains = 8; // tiles searched together by one lane (independent LDS reads in flight)

// TILE keys per sorted tile, a sample every QUANT keys (1024 / 256 straight from k_sel_tiles; 4096 / 512 after
// k_sel_merge4 for populations whose 1024-key tiles would be too many); R samples per lane = tiles * (TILE / QUANT) / 64
// LPK lanes share a key's searches, each kSelChains tiles at a time: 8 for the 64 tiles of the 1024-key layout, 4 for
// the <= 20 big tiles a pass stages (with 8, three quarters of the search chains would run empty)
template <uint32_t R, uint32_t TILE, uint32_t QUANT, uint32_t LPK>
__global__ __launch_bounds__(kSelThreads) void k_sel_rank_scatter(const uint32_t *__restrict__ kbits,
                                                                  const uint32_t *__restrict__ kidx,
                                                                  const uint32_t *__restrict__ samples,
                                                                  const float *__restrict__ vin,
                                                                  const float *__restrict__ sin,
                                                                  const float *__restrict__ fin,
                                                                  float *__restrict__ vout, float *__restrict__ sout,
                                                                  float *__restrict__ fout, uint32_t tiles, uint32_t need,
                                                                  uint32_t p_len, uint32_t d, SortExchange ex, uint32_t whole_tiles)
{
    constexpr uint32_t kWaves = kSelThreads / kWave;
    if (blockIdx.x == 0) ex_unpack(ex, vout, sout, fout, d, threadIdx.x, kSelThreads);
    // the names of the 1024 / 256 layout, shadowed by this instantiation's values
    constexpr uint32_t kSelTile = TILE, kSelQuantum = QUANT, kSelSamples = TILE / QUANT;
    // a tile whose prefix STARTS inside the window fits whole, skew included (at most window / QUANT tiles per pass)
    constexpr uint32_t kSelWindow = TILE == 1024 ? 33536 : 30720;
    static_assert(kSelWindow + kSelTile + kSelSkew * (kSelWindow / kSelQuantum) <= kSelCap, "staging buffer too small");
    static_assert(R * kWave <= kSelMaxTiles * sots::kSelSamples, "sample store too small");
    __shared__ __attribute__((aligned(16))) uint32_t staged[kSelCap];
    __shared__ __attribute__((aligned(16))) uint32_t smp[kSelMaxTiles * sots::kSelSamples], smi[kSelMaxTiles * sots::kSelSamples];
    __shared__ uint32_t off[kSelMaxTiles + 1]; // first staged position of each tile, all passes concatenated
    __shared__ uint16_t chunk_tile[kSelMaxTiles * sots::kSelSamples]; // tile of every QUANT staged positions
    // LDS place of tile t's prefix in its pass: off[t] - w0 + kSelSkew * (t - ta).  Prefix lengths are multiples
    // of 256 words, so without the skew every prefix would start on bank 0 and the first binary-search levels
    // (positions 511, 255, 127, 63, 31 of eight different tiles in one instruction) would all hit bank 31.
    __shared__ uint32_t own_bits[kSelMaxOwn], own_tile[kSelMaxOwn], own_pos[kSelMaxOwn], own_rank[kSelMaxOwn], own_src[kSelMaxOwn];
    __shared__ uint32_t wave_tot[kWaves];
    __shared__ unsigned long long vstar_s;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const uint32_t ns = tiles * kSelSamples;
    SOTS_PHASE_BEGIN();

    // ---- v* = the k-th smallest sample, k = ceil(need / 256), in (fitness bits, index) order: with the
    // index in the comparison, equal fitness values (a converged population is full of them) cannot
    // inflate the staged prefixes.  Every lane holds R = ns / 64 samples in registers; wavefront w ranks the
    // samples held by lanes 4w .. 4w+3: one sample at a time is broadcast as a SCALAR and compared with all
    // ns samples by R 64-bit vector compares whose lane masks are counted by s_bcnt1 - 64 comparisons per
    // vector instruction and no per-lane counters (a lane-per-pair count costs several times the vector work).
    // whole_tiles > 0 (a population of at most 8 real tiles, padded to 16): the real tiles are staged whole and the tiles of
    // padding not at all - no samples to fetch, no v* to rank (2.6 us in front of the copies), and every key's rank is exact
    if (whole_tiles == 0)
        for (uint32_t e = tid; e < ns; e += kSelThreads) {
            smp[e] = samples[e];
            smi[e] = samples[ns + e];
        }
    const uint32_t kth = (need + kSelQuantum - 1) / kSelQuantum;
    if (whole_tiles != 0) {
        if (tid == 0) vstar_s = ~0ull;
    } else if (kth > ns) {
        if (tid == 0) vstar_s = ~0ull; // more rows wanted than the samples can vouch for: stage everything
    } else {
        unsigned long long key[R]; // (bits << 32) | index: unique, so the ranks are a permutation
#pragma unroll
        for (uint32_t r = 0; r < R; ++r)
            key[r] = ((unsigned long long)samples[lane + kWave * r] << 32) | samples[ns + lane + kWave * r];
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) {
#pragma unroll
            for (uint32_t l = 0; l < 4; ++l) {
                const uint32_t src_lane = 4u * wave + l;
                const unsigned long long v = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(key[r] >> 32), (int)src_lane) << 32) |
                                             (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key[r], (int)src_lane);
                uint32_t below = 0;
#pragma unroll
                for (uint32_t r2 = 0; r2 < R; ++r2) below += (uint32_t)__popcll(__ballot(key[r2] < v));
                if (below == kth - 1 && lane == 0) vstar_s = v; // exactly one sample has this rank
            }
        }
    }
    __syncthreads();
    SOTS_PHASE(1);
    const uint32_t vstar_b = (uint32_t)(vstar_s >> 32), vstar_i = (uint32_t)vstar_s;

    // ---- staged prefix of every tile (256, 512, 768 or 1024 keys), exclusive scan -> off[] ---------
    {
        uint32_t quanta = 0; // prefix length / 256
        if (whole_tiles != 0) {
            quanta = tid < whole_tiles ? kSelSamples : 0u;
        } else if (tid < tiles) {
            uint32_t m = 0;
#pragma unroll
            for (uint32_t j = 0; j < kSelSamples; ++j) {
                const uint32_t sb = smp[tid * kSelSamples + j], si = smi[tid * kSelSamples + j];
                m += (sb < vstar_b || (sb == vstar_b && si <= vstar_i)) ? 1u : 0u;
            }
            quanta = m >= kSelSamples ? kSelSamples : m + 1u;
        }
        // prefix sum inside the wavefront from four ballots (quanta is 0..4), across wavefronts through LDS
        uint32_t before_lane = 0, wave_sum = 0;
#pragma unroll
        for (uint32_t q = 1; q <= kSelSamples; ++q) {
            const uint64_t mask = __ballot(quanta >= q);
            before_lane += __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            wave_sum += (uint32_t)__popcll(mask);
        }
        if (lane == 0) wave_tot[wave] = wave_sum;
        __syncthreads();
        uint32_t before = before_lane;
        for (uint32_t w = 0; w < wave; ++w) before += wave_tot[w];
        if (tid < tiles) {
            off[tid + 1] = (before + quanta) * kSelQuantum;
            for (uint32_t q = 0; q < quanta; ++q) chunk_tile[before + q] = (uint16_t)tid;
        }
        if (tid == 0) off[0] = 0;
    }
    __syncthreads();
    SOTS_PHASE(2);
    const uint32_t total = off[tiles];

    // ---- this workgroup's keys: an equal share of the staged positions.  Their fitness bits and row
    // indices are requested now and land while the prefixes are staged -------------------------------
    const uint32_t share = (total + gridDim.x - 1) / gridDim.x; // <= kSelMaxOwn by the launcher's grid
    uint32_t my_tile = 0xFFFFFFFFu, my_pos = 0, my_bits = 0xFFFFFFFFu, my_src = 0; // slot `tid`
    {
        const uint32_t g = blockIdx.x * share + tid;
        if (tid < share && g < total) {
            my_tile = chunk_tile[g / kSelQuantum];
            my_pos = g - off[my_tile];
            my_bits = kbits[(size_t)my_tile * kSelTile + my_pos];
            my_src = kidx[(size_t)my_tile * kSelTile + my_pos];
        }
    }
    SOTS_PHASE(3);

    // ---- passes over the staged prefixes ---------------------------------------------------------
    typedef __attribute__((address_space(3))) void *lds_ptr_t;
    const uint32_t sub = tid & (kSelLanesPerKey - 1);
    constexpr uint32_t kRowRounds = kSelMaxOwn / kSelKeysPerRound, kColsPerLane = (2 * SOTS_MAX_DIMS + 1 + kSelLanesPerKey - 1) / kSelLanesPerKey;
    float val[kRowRounds][kColsPerLane];
    const uint32_t passes = off[tiles - 1] / kSelWindow + 1;
    uint32_t ta = 0;
    for (uint32_t pass = 0; pass < passes; ++pass) {
        const uint32_t w0 = pass * kSelWindow;
        // first tile that starts at or beyond the end of this window: tiles [ta, tb) are staged
        uint32_t tb = tiles;
        if (w0 + kSelWindow < total) {
            const uint32_t t = chunk_tile[(w0 + kSelWindow) / kSelQuantum]; // the tile that owns that position
            tb = off[t] == w0 + kSelWindow ? t : t + 1;
        }
        if (pass) __syncthreads(); // the previous pass's searches are done with the staging buffer
        // wavefront w copies tiles ta + w, ta + w + 16, ...: lane m fetches the bounds of the m-th of them, then
        // the copies are issued back to back with wavefront-uniform (readlane) arguments
        {
            const uint32_t mine = ta + wave + lane * kWaves;
            const uint32_t b0 = mine < tb ? off[mine] : 0u, b1 = mine < tb ? off[mine + 1] : 0u;
            uint32_t m = 0;
            for (uint32_t tt = ta + wave; tt < tb; tt += kWaves, ++m) {
                const uint32_t o0 = (uint32_t)__builtin_amdgcn_readlane((int)b0, (int)m), o1 = (uint32_t)__builtin_amdgcn_readlane((int)b1, (int)m);
                const uint32_t *__restrict__ src = kbits + (size_t)tt * kSelTile;
                for (uint32_t e = 0; e < o1 - o0; e += 4 * kWave) // a multiple of 256: whole wavefront instructions
                    __builtin_amdgcn_global_load_lds(src + e + 4 * lane, (lds_ptr_t)(staged + (o0 - w0) + kSelSkew * (tt - ta) + e), 16, 0, 0);
            }
        }
        if (pass == 0) { // the own-key loads were issued before the copies, so they have landed too
            const bool live = my_tile != 0xFFFFFFFFu && my_bits != kSelPadBits; // padding keys move nothing
            if (tid < kSelMaxOwn) {
                own_tile[tid] = live ? my_tile : 0xFFFFFFFFu;
                own_pos[tid] = my_pos;
                own_bits[tid] = my_bits;
                own_src[tid] = my_src;
                own_rank[tid] = 0;
            }
        }
        SOTS_PHASE(4);
        __builtin_amdgcn_s_waitcnt(0); // vmcnt(0): this wavefront's copies have landed
        __syncthreads();
        SOTS_PHASE(5);
        if (pass == 0) {
            // the rows of this workgroup's keys are requested now, before it is known which of them made it (about
            // half do): the loads fly while the ranks are computed, eight lanes per key, lane `sub` holding row
            // elements sub, sub + 8, ...
#pragma unroll
            for (uint32_t r = 0; r < kRowRounds; ++r) {
                const uint32_t slot = r * kSelKeysPerRound + tid / kSelLanesPerKey;
                if (slot >= share || own_tile[slot] == 0xFFFFFFFFu) continue;
                const uint32_t src = own_src[slot];
#pragma unroll
                for (uint32_t q = 0; q < kColsPerLane; ++q) {
                    const uint32_t c = sub + q * kSelLanesPerKey;
                    if (c < d) val[r][q] = vin[(size_t)src * d + c];
                    else if (c < 2 * d) val[r][q] = sin[(size_t)src * d + (c - d)];
                    else if (c < 2 * d + 1) val[r][q] = fin[src];
                }
            }
        }
        for (uint32_t r0 = 0; r0 < share; r0 += kSelThreads / LPK) {
            const uint32_t slot = r0 + tid / LPK, ssub = tid % LPK;
            const uint32_t t_own = slot < share ? own_tile[slot] : 0xFFFFFFFFu;
            const bool live = t_own != 0xFFFFFFFFu;
            const uint32_t xb = live ? own_bits[slot] : 0u, pos_own = live ? own_pos[slot] : 0u;
            uint32_t count = 0;
            // kSelChains tiles per lane at a time, their binary searches advanced level by level.  A search keeps
            // the ABSOLUTE position in staged[] (one add less per step).
            for (uint32_t t0 = ta + ssub; t0 < tb; t0 += LPK * kSelChains) {
                uint32_t base[kSelChains], n[kSelChains], thr[kSelChains], p[kSelChains];
#pragma unroll
                for (uint32_t m = 0; m < kSelChains; ++m) {
                    const uint32_t tt = t0 + m * LPK;
                    const bool in = tt < tb && live;
                    const uint32_t o0 = in ? off[tt] : w0, o1 = in ? off[tt + 1] : w0;
                    base[m] = o0 - w0 + (in ? kSelSkew * (tt - ta) : 0u);
                    n[m] = o1 - o0;
                    thr[m] = in ? xb + (tt < t_own ? 1u : 0u) : 0u; // xb <= 0xFFFFFFFD for a live key: no wrap; never 0
                    p[m] = base[m];
                }
                // levels of a quantum or more: only while the step stays inside the prefix (prefix lengths are
                // multiples of the quantum, not powers of two)
#pragma unroll
                for (uint32_t step = kSelTile / 2; step >= kSelQuantum; step >>= 1) {
#pragma unroll
                    for (uint32_t m = 0; m < kSelChains; ++m)
                        p[m] += (p[m] + step <= base[m] + n[m] && staged[p[m] + step - 1] < thr[m]) ? step : 0u;
                }
                // a search that has reached the end of its prefix stops (threshold 0: nothing compares below it)
#pragma unroll
                for (uint32_t m = 0; m < kSelChains; ++m) thr[m] = p[m] - base[m] >= n[m] ? 0u : thr[m];
#pragma unroll
                for (uint32_t step = kSelQuantum / 2; step >= 1; step >>= 1) {
#pragma unroll
                    for (uint32_t m = 0; m < kSelChains; ++m) p[m] += staged[p[m] + step - 1] < thr[m] ? step : 0u;
                }
#pragma unroll
                for (uint32_t m = 0; m < kSelChains; ++m) {
                    const uint32_t tt = t0 + m * LPK;
                    const uint32_t lb = p[m] - base[m] + (staged[p[m]] < thr[m] ? 1u : 0u);
                    count += (tt == t_own && tt < tb) ? pos_own : lb; // the own tile counts in the pass that stages it
                }
            }
            count += lane_xor<1>(count);
            if constexpr (LPK >= 4) count += lane_xor<2>(count);
            if constexpr (LPK == 8) count += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)count, 0x141, 0xf, 0xf, false); // row_half_mirror
            static_assert(LPK == 2 || LPK == 4 || LPK == 8, "the partial counts are added over 2, 4 or 8 neighbouring lanes");
            if (ssub == 0 && live) own_rank[slot] += count; // one writer per slot
        }
        ta = tb;
    }
    __syncthreads();
    SOTS_PHASE(6);

    // ---- rows of the keys that made it (requested above) -------------------------------------------
    const uint32_t width = 2 * d + 1;
#pragma unroll
    for (uint32_t r = 0; r < kRowRounds; ++r) {
        const uint32_t slot = r * kSelKeysPerRound + tid / kSelLanesPerKey;
        if (slot >= share || own_tile[slot] == 0xFFFFFFFFu) continue;
        const uint32_t dst = own_rank[slot];
        if (dst >= need || ex_immigrant_row(ex, dst)) continue;
#pragma unroll
        for (uint32_t q = 0; q < kColsPerLane; ++q) {
            const uint32_t c = sub + q * kSelLanesPerKey;
            if (c < d) vout[(size_t)dst * d + c] = val[r][q];
            else if (c < 2 * d) sout[(size_t)dst * d + (c - d)] = val[r][q];
            else if (c < width) fout[dst] = val[r][q];
            if (c < width) ex_sink(ex, dst, c, d, val[r][q]);
        }
    }
    SOTS_PHASE(7);
}

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
