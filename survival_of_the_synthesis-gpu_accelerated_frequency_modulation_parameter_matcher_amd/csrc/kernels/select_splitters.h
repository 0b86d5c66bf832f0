// select_splitters.h -- the selection in one launch, ranked between the previous generation's splitters (k_sel_splitters),
// and the kernel that seeds the splitter slot after a two-launch selection (k_sel_seed).
#pragma once
#include "common.h"
#include "sel_keys.h"
#include "sort.h"
#include "stamps.h"

// contraction: off (the translation unit's default: the stream compares floats and never computes with them)
#pragma clang fp contract(off)
namespace sots { namespace {

// ------------------------------------------------------------------------------------
// The selection in ONE launch, ranked between stored splitters.
//
// Keys are (order_bits(fitness) << 32) | row index: unique, ties by index, NaN last.  The slot holds B = gridDim.x
// 64-bit splitters; every workgroup makes them non-decreasing the same way (t_0 = 0, running maximum), so the buckets
// [t_j, t_{j+1}) - the last one open - are disjoint and cover every key WHATEVER the slot holds.  Workgroup j streams
// all P fitness values once, counts the keys below t_j (c_j) and collects the keys of its bucket in LDS, sorts that
// list (bitonic network in LDS) and has every key's final position: c_j + its place in the list.  Rows with a position
// below `need` move; the keys at positions q * step become the next launch's splitters, written to the OTHER slot.
// Good splitters (the previous generation's, a generation moves the distribution little) make small buckets; bad ones
// only cost time: a bucket that outgrows the LDS list is collected again into keys_scratch[c_j ...] (the buckets'
// places in the final order, so disjoint) and sorted there by its workgroup alone.  No workgroup waits for another.
//
// The stream compares in the float domain where both bounds are the bits of numbers: f < bound is order_bits(f) <
// bits(bound), NaN compares false as its key lies above every number, and -0 = +0 both ways; the row index decides only
// where a fitness EQUALS a bound (one wavefront-uniform branch).  Bounds above +inf (NaN keys, 0xFFFF...) take the
// 64-bit compare.
// ------------------------------------------------------------------------------------
constexpr uint32_t kSplThreads = 1024;
constexpr uint32_t kSplCap = 8192;       // keys of the LDS list (64 KiB)
constexpr uint32_t kSplMaxBuckets = 1024; // splitters per slot (the grid is one workgroup per CU)
constexpr uint32_t kSplAhead = 16;        // 16-byte loads per lane requested up front (64 registers)
__device__ __forceinline__ float spl_bound_float(uint64_t t) // of a normalised bound with numeric bits
{
    const uint32_t b = (uint32_t)(t >> 32);
    return __uint_as_float((b & 0x80000000u) ? b ^ 0x80000000u : ~b);
}

struct SplScan {
    uint64_t lo, hi;
    float lo_f, hi_f;
    bool last; // the open bucket: no upper bound
};

// one key per lane: counts the keys below lo, appends the bucket's keys (LDS list while it has room; to `spill`, the
// second time round, all of them)
template <bool FLOATS>
__device__ __forceinline__ void spl_visit(const SplScan &s, float f, uint32_t idx, bool valid, uint32_t &below,
                                          uint32_t *__restrict__ n_s, uint64_t *__restrict__ list, uint64_t *__restrict__ spill)
{
    uint64_t b_lo, b_hi;
    if constexpr (FLOATS) {
        b_lo = __ballot(f < s.lo_f);
        b_hi = s.last ? ~0ull : __ballot(f < s.hi_f);
        const uint64_t eq_lo = __ballot(f == s.lo_f), eq_hi = s.last ? 0ull : __ballot(f == s.hi_f);
        if (eq_lo | eq_hi) { // wavefront-uniform: somebody's fitness equals a bound, the index decides
            b_lo |= eq_lo & __ballot(idx < (uint32_t)s.lo);
            b_hi |= eq_hi & __ballot(idx < (uint32_t)s.hi);
        }
    } else {
        const uint64_t key = sel_key(f, idx);
        b_lo = __ballot(valid && key < s.lo);
        b_hi = __ballot(valid && (s.last || key < s.hi));
    }
    below += (uint32_t)__popcll(b_lo);
    const uint64_t in = b_hi & ~b_lo;
    if (in) {
        const uint32_t lane = threadIdx.x & (kWave - 1);
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(n_s, (uint32_t)__popcll(in));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(in >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)in, 0u));
        if ((in >> lane) & 1ull) {
            const uint64_t key = sel_key(f, idx);
            if (spill) spill[slot] = key;
            else if (slot < kSplCap) list[slot] = key;
        }
    }
}

// all P keys past one workgroup; returns the wavefront's count of keys below lo
template <bool FLOATS>
__device__ __forceinline__ uint32_t spl_stream(const SplScan &s, const float *__restrict__ fin, uint32_t p_len, bool vec, uint32_t first,
                                               uint32_t *__restrict__ n_s, uint64_t *__restrict__ list, uint64_t *__restrict__ spill)
{
    constexpr uint32_t kPerIter = 4 * kSplThreads, kBatch = 4;
    const uint32_t tid = threadIdx.x;
    uint32_t below = 0, done = first; // keys in front of `first` are done (vec: first == 0)
    if (vec) { // whole iterations of 16 bytes per lane, four loads in flight
        const uint32_t full = p_len / kPerIter;
        uint32_t it = 0;
        for (; it + kBatch <= full; it += kBatch) {
            float4 q[kBatch];
#pragma unroll
            for (uint32_t u = 0; u < kBatch; ++u) q[u] = *reinterpret_cast<const float4 *>(fin + (size_t)(it + u) * kPerIter + 4 * tid);
#pragma unroll
            for (uint32_t u = 0; u < kBatch; ++u) {
                const uint32_t i0 = (it + u) * kPerIter + 4 * tid;
                spl_visit<FLOATS>(s, q[u].x, i0, true, below, n_s, list, spill);
                spl_visit<FLOATS>(s, q[u].y, i0 + 1, true, below, n_s, list, spill);
                spl_visit<FLOATS>(s, q[u].z, i0 + 2, true, below, n_s, list, spill);
                spl_visit<FLOATS>(s, q[u].w, i0 + 3, true, below, n_s, list, spill);
            }
        }
        for (; it < full; ++it) {
            const uint32_t i0 = it * kPerIter + 4 * tid;
            const float4 q = *reinterpret_cast<const float4 *>(fin + i0);
            spl_visit<FLOATS>(s, q.x, i0, true, below, n_s, list, spill);
            spl_visit<FLOATS>(s, q.y, i0 + 1, true, below, n_s, list, spill);
            spl_visit<FLOATS>(s, q.z, i0 + 2, true, below, n_s, list, spill);
            spl_visit<FLOATS>(s, q.w, i0 + 3, true, below, n_s, list, spill);
        }
        done = full * kPerIter;
    }
    // the rest one key per lane, with the 64-bit compare (it takes the lanes beyond the end as well)
    for (uint32_t i0 = done; i0 < p_len; i0 += kSplThreads) { // workgroup-uniform trip count
        const uint32_t idx = i0 + tid;
        const bool valid = idx < p_len;
        const float f = valid ? fin[idx] : 0.0f;
        spl_visit<false>(s, f, idx, valid, below, n_s, list, spill);
    }
    return below;
}

// ---- the stream where both bounds are numbers: per key one compare and a per-lane count for "below lo", one compare
// for "not above hi"; the keys that pass both - the bucket's, and the ties with either bound - are then decided by
// their 64-bit keys.
// a lane whose key passed both float compares (lo_f <= f <= hi_f): the bucket's, or a tie with one of the bounds, where
// the row index decides - key < lo only if f == lo_f and the index is below lo's, key < hi unless f == hi_f and the index
// is not below hi's.  A converged population ties by the thousand: every lane comes through here then.
__device__ __forceinline__ void spl_candidate(const SplScan &s, float f, uint32_t idx, uint32_t &cnt, uint32_t *__restrict__ n_s,
                                              uint64_t *__restrict__ list)
{
    const bool below = f == s.lo_f && idx < (uint32_t)s.lo;
    cnt += below ? 1u : 0u;
    if (!below && (f < s.hi_f || idx < (uint32_t)s.hi)) {
        const uint32_t slot = atomicAdd(n_s, 1u);
        if (slot < kSplCap) list[slot] = sel_key(f, idx);
    }
}
template <bool COUNT_ONLY>
__device__ __forceinline__ void spl_fast4(const SplScan &s, const float4 q, uint32_t i0, uint32_t &cnt, uint32_t *__restrict__ n_s,
                                          uint64_t *__restrict__ list)
{
    const bool l0 = q.x < s.lo_f, l1 = q.y < s.lo_f, l2 = q.z < s.lo_f, l3 = q.w < s.lo_f;
    cnt += (l0 ? 1u : 0u) + (l1 ? 1u : 0u) + (l2 ? 1u : 0u) + (l3 ? 1u : 0u);
    if constexpr (COUNT_ONLY) { // the ties with lo that lie below it: by the row index
        const uint32_t li = (uint32_t)s.lo;
        const bool e0 = q.x == s.lo_f, e1 = q.y == s.lo_f, e2 = q.z == s.lo_f, e3 = q.w == s.lo_f;
        if (e0 | e1 | e2 | e3)
            cnt += (e0 && i0 < li ? 1u : 0u) + (e1 && i0 + 1 < li ? 1u : 0u) + (e2 && i0 + 2 < li ? 1u : 0u) + (e3 && i0 + 3 < li ? 1u : 0u);
    } else {
        // per lane, no ballots: a few lanes of a few wavefront instructions have a candidate while the splitters are good
        const bool c0 = !l0 && q.x <= s.hi_f, c1 = !l1 && q.y <= s.hi_f, c2 = !l2 && q.z <= s.hi_f, c3 = !l3 && q.w <= s.hi_f;
        if (c0 | c1 | c2 | c3) {
            if (c0) spl_candidate(s, q.x, i0, cnt, n_s, list);
            if (c1) spl_candidate(s, q.y, i0 + 1, cnt, n_s, list);
            if (c2) spl_candidate(s, q.z, i0 + 2, cnt, n_s, list);
            if (c3) spl_candidate(s, q.w, i0 + 3, cnt, n_s, list);
        }
    }
}
// the whole iterations of 16 bytes per lane (`full` of them).  The first kSplAhead were requested by the caller, all at
// once, before it did anything else: with one or two kilobytes in flight per wavefront the stream ran at the latency of
// four dependent batches, four times the time the data takes to arrive.  A population of 65 536 is exactly kSplAhead.
template <bool COUNT_ONLY>
__device__ __forceinline__ uint32_t spl_stream_fast(const SplScan &s, const float *__restrict__ fin, uint32_t full, const float4 (&pre)[kSplAhead],
                                                    uint32_t &cnt, uint32_t *__restrict__ n_s, uint64_t *__restrict__ list)
{
    constexpr uint32_t kPerIter = 4 * kSplThreads;
    const uint32_t tid = threadIdx.x;
#pragma unroll
    for (uint32_t u = 0; u < kSplAhead; ++u)
        if (u < full) spl_fast4<COUNT_ONLY>(s, pre[u], u * kPerIter + 4 * tid, cnt, n_s, list);
    for (uint32_t it = kSplAhead; it < full; ++it) {
        const uint32_t i0 = it * kPerIter + 4 * tid;
        spl_fast4<COUNT_ONLY>(s, *reinterpret_cast<const float4 *>(fin + i0), i0, cnt, n_s, list);
    }
    return full * kPerIter;
}

// ---- ordering up to 1024 keys, one per lane: the distances below 64 are lane exchanges in registers (k_sel_tiles'
// network, kernels/select_tiles.h, with the direction as an argument), the others go through LDS, written to one of two buffers in turn so
// that a step needs one barrier
template <uint32_t J>
__device__ __forceinline__ void spl_reg_merge(uint32_t &b, uint32_t &i, uint32_t lane, bool asc)
{
    const uint32_t pb = lane_xor<J>(b), pi = lane_xor<J>(i);
    const bool keep_min = ((lane & J) == 0) == asc;
    const bool mine_less = b < pb || (b == pb && i < pi);
    if (keep_min != mine_less) {
        b = pb;
        i = pi;
    }
    if constexpr (J > 1) spl_reg_merge<J / 2>(b, i, lane, asc);
}

__device__ __forceinline__ void spl_cmp_swap(uint64_t *__restrict__ a, uint32_t i, uint32_t l, bool ascending)
{
    const uint64_t x = a[i], y = a[l];
    if ((x > y) == ascending) {
        a[i] = y;
        a[l] = x;
    }
}

__global__ __launch_bounds__(kSplThreads) void k_sel_splitters(const float *__restrict__ vin, const float *__restrict__ sin,
                                                                const float *__restrict__ fin, float *__restrict__ vout,
                                                                float *__restrict__ sout, float *__restrict__ fout,
                                                                const uint64_t *__restrict__ spl_in, uint64_t *__restrict__ spl_out,
                                                                uint64_t *__restrict__ keys_scratch, uint32_t p_len, uint32_t need,
                                                                uint32_t step, uint32_t d, SortExchange ex, uint32_t vec, SelLists bk)
{
    __shared__ __attribute__((aligned(16))) uint64_t list[kSplCap];
    __shared__ unsigned long long bound_s[2];
    __shared__ uint32_t n_s, c_s;
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint32_t B = gridDim.x, j = blockIdx.x;
    if (j == 0) ex_unpack(ex, vout, sout, fout, d, tid, kSplThreads);
    SOTS_PHASE_BEGIN();
    // the slot, then the stream, are requested before anything else (loads return in order: the bounds are made while the
    // keys arrive)
    const unsigned long long my_spl = tid && tid <= j + 1 && tid < B ? spl_in[tid] : 0ull; // B <= kSplThreads
    // LIST MODE (bk.cnt): the kernel that made the fitness has filed every key under its bucket between these same
    // splitters.  Instead of the stream: the closed buckets' counters - c is the sum of those in front, n the own one, the
    // open bucket's the rest of P - and the own list, asked for at its full capacity before n is known (what lies
    // beyond n is an older generation's and is never looked at).  The set the NEXT generation counts into is cleared here.
    const bool by_list = bk.cnt != nullptr;
    constexpr uint32_t kShardWords = kSelListShards / 4; // a bucket's counters, 16 bytes at a time
    uint4 cnt_q[kShardWords], own_q[kShardWords];        // bucket tid's / this workgroup's own
#pragma unroll
    for (uint32_t w = 0; w < kShardWords; ++w) {
        cnt_q[w] = by_list && tid + 1 < B ? reinterpret_cast<const uint4 *>(bk.cnt)[tid * kShardWords + w] : uint4{0u, 0u, 0u, 0u};
        own_q[w] = by_list ? reinterpret_cast<const uint4 *>(bk.cnt)[j * kShardWords + w] : uint4{0u, 0u, 0u, 0u};
    }
    uint64_t pre_list[kSelListCap / kSplThreads];
#pragma unroll
    for (uint32_t u = 0; u < kSelListCap / kSplThreads; ++u) pre_list[u] = by_list ? bk.lists[(size_t)j * kSelListCap + u * kSplThreads + tid] : 0ull;
    if (by_list && tid < kSelListShards) bk.cnt_other[j * kSelListShards + tid] = 0u;
    uint32_t my_cnt = 0;
#pragma unroll
    for (uint32_t w = 0; w < kShardWords; ++w) my_cnt += cnt_q[w].x + cnt_q[w].y + cnt_q[w].z + cnt_q[w].w;
    const uint32_t full = (vec & 1u) ? p_len / (4 * kSplThreads) : 0u, ahead = by_list ? 0u : full;
    float4 pre[kSplAhead];
#pragma unroll
    for (uint32_t u = 0; u < kSplAhead; ++u) pre[u] = u < ahead ? *reinterpret_cast<const float4 *>(fin + (size_t)u * 4 * kSplThreads + 4 * tid) : float4{0.f, 0.f, 0.f, 0.f};

    // ---- this workgroup's bounds: the running maximum of the slot up to j and up to j + 1, t_0 = 0 --------------
    if (tid < 2) bound_s[tid] = 0;
    if (tid == 0) n_s = 0, c_s = 0;
    __syncthreads();
    {
        unsigned long long lo = tid <= j ? my_spl : 0ull, hi = my_spl;
#pragma unroll
        for (int m = kWave / 2; m >= 1; m >>= 1) {
            const unsigned long long l2 = __shfl_xor(lo, m), h2 = __shfl_xor(hi, m);
            lo = l2 > lo ? l2 : lo;
            hi = h2 > hi ? h2 : hi;
        }
        if (lane == 0 && hi != 0) { // (a wavefront with nothing to add holds zeros)
            atomicMax(&bound_s[0], lo);
            atomicMax(&bound_s[1], hi);
        }
    }
    if (by_list) {
        uint32_t in_front = tid < j ? my_cnt : 0u;
#pragma unroll
        for (int m = kWave / 2; m >= 1; m >>= 1) in_front += __shfl_xor(in_front, m);
        if (lane == 0 && in_front) atomicAdd(&c_s, in_front);
        if (tid == j) n_s = my_cnt; // (the open bucket: 0 here, P - c below)
        static_assert(kSelListSeg * kSelListShards == kSelListCap && kSelListShards % 4 == 0 && kSplThreads % kSelListSeg == 0, "segments");
    }
    __syncthreads();
    SplScan s;
    s.last = j + 1 == B;
    s.lo = spl_normalise(bound_s[0]);
    s.hi = spl_normalise(bound_s[1]);
    const bool floats = (uint32_t)(s.lo >> 32) <= kSplBitsPosInf && (s.last || (uint32_t)(s.hi >> 32) <= kSplBitsPosInf);
    s.lo_f = floats ? spl_bound_float(s.lo) : 0.0f;
    s.hi_f = floats && !s.last ? spl_bound_float(s.hi) : 0.0f;
    SOTS_PHASE(1);

    // ---- the stream ---------------------------------------------------------------------------------------------
    // The open bucket (the last workgroup) only counts on its way through: it holds whatever lies beyond the last
    // splitter - most of the population when the splitters are good - and is looked at only if positions below `reach`
    // fall into it.
    const bool count_only = !by_list && floats && s.last;
    const uint32_t reach = (B - 1) * step + 1 > need ? (B - 1) * step + 1 : need;
    bool stream = !by_list;
    if (by_list) {
        // The list serves unless it overflowed, or the bucket is the open one and has rows to place (nobody files the open
        // bucket).  Then this workgroup alone streams as without lists - counting and collecting by the 64-bit keys, into
        // the LDS list while it has room - which is exact for every slot; the counters are a promise of speed only.
        const uint32_t c0 = c_s, n0 = s.last ? p_len - c0 : n_s;
        const bool owes = n0 != 0 && c0 < reach && !(s.last && c0 >= need);
        // the segments one behind the other: place `at` of segment g goes to (keys of the segments in front) + at
        const uint32_t own[kSelListShards] = {own_q[0].x, own_q[0].y, own_q[0].z, own_q[0].w, own_q[1].x, own_q[1].y, own_q[1].z, own_q[1].w,
                                              own_q[2].x, own_q[2].y, own_q[2].z, own_q[2].w, own_q[3].x, own_q[3].y, own_q[3].z, own_q[3].w};
        static_assert(kSelListShards == 16, "own[] spells the sixteen counters out");
        bool overflow = false;
#pragma unroll
        for (uint32_t g = 0; g < kSelListShards; ++g) overflow |= own[g] > kSelListSeg;
        stream = owes && (s.last || overflow);
        if (owes && !stream) {
#pragma unroll
            for (uint32_t u = 0; u < kSelListCap / kSplThreads; ++u) {
                const uint32_t g0 = (u * kSplThreads + tid) / kSelListSeg, at = tid % kSelListSeg; // (kSplThreads is a multiple of the segment)
                uint32_t front = 0, mine = 0;
#pragma unroll
                for (uint32_t g = 0; g < kSelListShards; ++g) {
                    front += g < g0 ? own[g] : 0u;
                    mine = g == g0 ? own[g] : mine;
                }
                if (at < mine) list[front + at] = pre_list[u];
            }
        }
        __syncthreads(); // (everybody has read c_s and n_s)
        if (stream && tid == 0) n_s = 0, c_s = 0;
        if (stream) __syncthreads();
    }
    if (stream) {
        uint32_t cnt = 0, done = 0;
        if (!by_list && floats && (vec & 1u)) { // (list mode has not asked for `pre`)
            done = count_only ? spl_stream_fast<true>(s, fin, full, pre, cnt, &n_s, list)
                              : spl_stream_fast<false>(s, fin, full, pre, cnt, &n_s, list);
#pragma unroll
            for (int m = kWave / 2; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
        }
        if (done < p_len || !floats) cnt += spl_stream<false>(s, fin, p_len, (vec & 1u) != 0 && done == 0, done, &n_s, list, nullptr);
        if (lane == 0 && cnt) atomicAdd(&c_s, cnt);
    }
    __syncthreads();
    SOTS_PHASE(2);
    const uint32_t c = c_s, n = count_only || (by_list && !stream && s.last) ? p_len - c : n_s;
    // positions [c, c + n) are this workgroup's: rows to move below `need`, splitters to write at q * step, q < B
    if (j == 0 && tid == 0) spl_out[0] = 0;
    if (n == 0 || c >= reach) return;
    if (s.last && c >= need) {
        // The open bucket moves no row and only owes the splitters whose positions fall into it.  It keeps its own lower
        // bound for them instead of ordering what may be most of the population: a splitter may be ANY key, and this one
        // stays the last while the cut stays in front of it (a converged population whose keys all tie puts exactly as many
        // keys below it every generation: position (B - 1) * step is then always the open bucket's first)
        for (uint32_t q = (c + step - 1) / step + tid; q < B; q += kSplThreads)
            if (q) spl_out[q] = s.lo;
        return;
    }
    if (count_only || n > kSplCap) {
        // the bucket (again): into the LDS list if it fits, else - the slow path - into its place in the scratch keys
        __syncthreads();
        if (tid == 0) n_s = 0;
        __syncthreads();
        (void)spl_stream<false>(s, fin, p_len, (vec & 1u) != 0, 0, &n_s, list, n > kSplCap ? keys_scratch + c : nullptr);
        __syncthreads();
    }

    const uint64_t *sorted = list;
    uint32_t my_src = 0; // one key per lane: the row of the key at place tid
    if (n <= kSplThreads) {
        // ---- one key per lane (the usual case)
        uint32_t kb = 0xFFFFFFFFu, ki = 0xFFFFFFFFu; // beyond n: above every key
        if (tid < n) {
            const uint64_t key = list[tid];
            kb = (uint32_t)(key >> 32);
            ki = (uint32_t)key;
        }
        __syncthreads(); // the list is in registers: its first 2048 places are the two exchange buffers now
        uint32_t n_pad = kWave, buf = 0;
        while (n_pad < n) n_pad <<= 1;
        const bool busy = tid < n_pad; // wavefront-uniform: the others hold nothing but padding and only keep the barriers
        if (busy) {
            spl_reg_merge<1>(kb, ki, lane, (tid & 2u) == 0);
            spl_reg_merge<2>(kb, ki, lane, (tid & 4u) == 0);
            spl_reg_merge<4>(kb, ki, lane, (tid & 8u) == 0);
            spl_reg_merge<8>(kb, ki, lane, (tid & 16u) == 0);
            spl_reg_merge<16>(kb, ki, lane, (tid & 32u) == 0);
            spl_reg_merge<32>(kb, ki, lane, (tid & 64u) == 0);
        }
        for (uint32_t k = 2 * kWave; k <= n_pad; k <<= 1) {
            const bool asc = (tid & k) == 0;
            for (uint32_t jj = k >> 1; jj >= kWave; jj >>= 1) {
                list[buf * kSplThreads + tid] = ((uint64_t)kb << 32) | ki;
                __syncthreads();
                const uint64_t other = list[buf * kSplThreads + (tid ^ jj)];
                buf ^= 1u; // the next step writes the other buffer: nobody waits for this step's readers
                const uint64_t mine = ((uint64_t)kb << 32) | ki;
                if ((((tid & jj) == 0) == asc) != (mine < other)) {
                    kb = (uint32_t)(other >> 32);
                    ki = (uint32_t)other;
                }
            }
            if (busy) spl_reg_merge<32>(kb, ki, lane, asc);
        }
        list[buf * kSplThreads + tid] = ((uint64_t)kb << 32) | ki;
        my_src = ki;
        __syncthreads();
        sorted = list + buf * kSplThreads;
    } else if (n <= kSplCap) {
        // ---- bitonic network over the LDS list, padded with keys above every key.  A step whose distance stays inside
        // 64 pairs touches only the 128 keys its wavefront touched in the step before: no workgroup barrier between two
        // such steps
        uint32_t n_pad = 2;
        while (n_pad < n) n_pad <<= 1;
        for (uint32_t i = n + tid; i < n_pad; i += kSplThreads) list[i] = ~0ull;
        bool prev_local = false;
        for (uint32_t k = 2; k <= n_pad; k <<= 1) {
            for (uint32_t jj = k >> 1; jj > 0; jj >>= 1) {
                const bool local = jj <= kWave / 2;
                if (prev_local && local) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                } else {
                    __syncthreads();
                }
                prev_local = local;
                for (uint32_t pr = tid; pr < n_pad / 2; pr += kSplThreads) {
                    const uint32_t i = ((pr & ~(jj - 1)) << 1) | (pr & (jj - 1));
                    spl_cmp_swap(list, i, i + jj, (i & k) == 0);
                }
            }
        }
        __syncthreads();
    } else {
        // ---- the slow path: the bucket in its place in the scratch keys, ordered there by an ascending
        // network whose missing upper end counts as keys above every key (pairs that reach beyond n are no-ops)
        uint64_t *g = keys_scratch + c; // (collected above)
        uint32_t n_pad = 2, log2k = 1;
        while (n_pad < n) n_pad <<= 1;
        for (uint32_t k = 2; k <= n_pad; k <<= 1, ++log2k) {
            __syncthreads();
            for (uint32_t pr = tid; pr < n_pad / 2; pr += kSplThreads) { // first step of a merge: i against its mirror in the block
                const uint32_t blk = pr >> (log2k - 1), x = pr & ((k >> 1) - 1);
                const uint32_t i = blk * k + x, l = blk * k + (k - 1 - x);
                if (l < n) spl_cmp_swap(g, i, l, true);
            }
            for (uint32_t jj = k >> 2; jj > 0; jj >>= 1) {
                __syncthreads();
                for (uint32_t pr = tid; pr < n_pad / 2; pr += kSplThreads) {
                    const uint32_t i = ((pr & ~(jj - 1)) << 1) | (pr & (jj - 1));
                    if (i + jj < n) spl_cmp_swap(g, i, i + jj, true);
                }
            }
        }
        __syncthreads();
        sorted = g;
    }
    SOTS_PHASE(3);

    // ---- next launch's splitters: the keys at positions q * step, 1 <= q < B -----------------------------------------
    {
        const uint32_t q0 = c == 0 ? 1u : (c + step - 1) / step;
        for (uint32_t q = q0 + tid; q < B && (uint64_t)q * step < (uint64_t)c + n; q += kSplThreads) spl_out[q] = sorted[q * step - c];
    }
    // ---- rows ----------------------------------------------------------------------------------------------------
    if (c >= need) return;
    const uint32_t rows = need - c < n ? need - c : n, width = 2 * d + 1;
    if (n <= kSplThreads && d == 4 && (vec & 2u)) {
        // a lane per row, its key still in registers: all of a row's loads are in flight together (16-byte rows)
        const uint32_t dst = c + tid;
        if (tid < rows && !ex_immigrant_row(ex, dst)) {
            const float4 v = reinterpret_cast<const float4 *>(vin)[my_src], t = reinterpret_cast<const float4 *>(sin)[my_src];
            const float f = fin[my_src];
            reinterpret_cast<float4 *>(vout)[dst] = v;
            reinterpret_cast<float4 *>(sout)[dst] = t;
            fout[dst] = f;
            if (dst < ex.sink_rows) {
                const float row[9] = {v.x, v.y, v.z, v.w, t.x, t.y, t.z, t.w, f};
#pragma unroll
                for (uint32_t col = 0; col < 9; ++col) ex_sink(ex, dst, col, d, row[col]);
            }
        }
        SOTS_PHASE(4);
        return;
    }
    for (uint32_t e = tid; e < rows * width; e += kSplThreads) {
        const uint32_t r = e / width, col = e - r * width, dst = c + r;
        if (ex_immigrant_row(ex, dst)) continue;
        const uint32_t src = (uint32_t)sorted[r];
        float v;
        if (col < d) v = vin[(size_t)src * d + col];
        else if (col < 2 * d) v = sin[(size_t)src * d + (col - d)];
        else v = fin[src];
        if (col < d) vout[(size_t)dst * d + col] = v;
        else if (col < 2 * d) sout[(size_t)dst * d + (col - d)] = v;
        else fout[dst] = v;
        ex_sink(ex, dst, col, d, v);
    }
    SOTS_PHASE(4);
}

// the splitter slot after the two-launch selection: the sorted fitness it wrote, at the same rank step (a splitter
// needs no index: any value does, the order of the slot is what makes the buckets small)
__global__ __launch_bounds__(kSplMaxBuckets) void k_sel_seed(const float *__restrict__ fsorted, uint64_t *__restrict__ spl_out,
                                                             uint32_t need, uint32_t step, uint32_t buckets)
{
    const uint32_t q = threadIdx.x;
    if (q >= buckets) return;
    const uint32_t pos = q * step < need ? q * step : need - 1;
    spl_out[q] = q ? (uint64_t)order_bits(fsorted[pos]) << 32 : 0ull;
}

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
