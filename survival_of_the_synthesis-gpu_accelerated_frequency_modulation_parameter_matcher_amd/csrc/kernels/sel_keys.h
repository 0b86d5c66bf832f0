// sel_keys.h -- the 64-bit selection key of a row (order_bits, sel_key), the normalised splitter and the bucket of a key
// between the splitters of a slot (bkt_bounds, bkt_flush, bkt_visit): what the sort, the selection and the key-filing
// spectral kernel share.
#pragma once
#include "common.h"
#include "../sots_bkt_layout.h"

// contraction: on, as where this code stood - between the transform and k_fft, which inlines bkt_visit.  Nothing here
// multiplies and adds floats; the mode is kept so that the file is the code it was, to the byte
#pragma clang fp contract(on)
namespace sots { namespace {

// ------------------------------------------------------------------------------------
// Selection keys, and the bucket of a key between the splitters of a slot (list mode).  They stand in
// front of the spectral kernel because k_fft<.., BUCKET = true> files every row's key under its bucket as soon as it
// has the row's fitness: the selection then reads its bucket's keys from a list instead of streaming all P.
// ------------------------------------------------------------------------------------
// order-preserving bits of a fitness: every number (at most 0xFF800000, +inf) below NaN (0xFFFFFFFD), NaN
// below the padding key (0xFFFFFFFE); 0xFFFFFFFF stays free so that "bits + 1" never wraps
constexpr uint32_t kSelPadBits = 0xFFFFFFFEu;
__device__ __forceinline__ uint32_t order_bits(float f)
{
    if (f != f) return 0xFFFFFFFDu;
    const uint32_t u = __float_as_uint(f == 0.0f ? 0.0f : f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

constexpr uint32_t kSplBitsNegInf = 0x007FFFFFu, kSplBitsPosInf = 0xFF800000u; // order_bits(-inf), order_bits(+inf)

__device__ __forceinline__ uint64_t sel_key(float f, uint32_t idx) { return ((uint64_t)order_bits(f) << 32) | idx; }

// the least key that is >= t and that compares like t against every key that exists: bits below -inf's hold no key, and
// neither does 0x7FFFFFFF (-0 is keyed as +0)
__device__ __forceinline__ uint64_t spl_normalise(uint64_t t)
{
    const uint32_t b = (uint32_t)(t >> 32);
    if (b < kSplBitsNegInf) return (uint64_t)kSplBitsNegInf << 32;
    if (b == 0x7FFFFFFFu) return (uint64_t)0x80000000u << 32;
    return t;
}

constexpr uint32_t kBktMaxBuckets = kSelListMaxBuckets; // bounds a bucketing workgroup keeps in LDS (2 KiB)
static_assert(kBktMaxBuckets % kWave == 0, "a lane looks at kBktMaxBuckets / 64 bounds");

// How a filing kernel finds the bucket of a key, a compile-time choice of its instantiation (the host's one rule:
// bkt_two_level(), sots_kernels.hip).  Both count the bounds at or below the key and name the same bucket for every key
// and every slot content.
//   kBktFlat: all kBktMaxBuckets bounds against every key, fitness bits first and the row indices on a tie.
//   kBktTwoLevel: the open bucket first (one compare of two scalar pairs), else 64 group ends and then the four bounds of
//   one group, whole 64-bit keys: two LDS reads, no tie path.
constexpr int kBktFlat = 0, kBktTwoLevel = 1;
// the lists argument of a kernel that files by two levels: the lookup travels in the argument's type, so the flat
// instantiations keep their names and their code
struct SelListsTwoLevel : SelLists {};
template <typename L> constexpr int bkt_lookup_of = std::is_same_v<L, SelListsTwoLevel> ? kBktTwoLevel : kBktFlat;
// the lists type among a kernel's trailing arguments (the first of them, where it has lists), SelLists where it has none
template <typename... A> struct bkt_lists_of { using type = SelLists; };
template <typename A, typename... R> struct bkt_lists_of<A, R...> { using type = std::conditional_t<std::is_base_of_v<SelLists, A>, A, SelLists>; };
static_assert(kBktGroups * kBktGroupSize == kBktMaxBuckets && kBktGroups == kWave, "a lane per group of bounds");

// The slot made non-decreasing exactly as k_sel_splitters makes it (t_0 = 0, running maximum, spl_normalise), into
// bnd: ONE wavefront, in front of a workgroup barrier.
// kBktFlat: bound q's fitness bits lie at bnd[q], its row index at bnd[kBktMaxBuckets + q].  Bound 0 and those from B on
// are ~0, a bound no key reaches: the bucket of a key is then the number of bounds t_q <= key.
// kBktTwoLevel: bnd holds whole keys, bound q at bkt_slot_of(q) (sots_bkt_layout.h).  Bound 0 is 0 - at or below every
// key, and taken off the count again - and those from B on are ~0: the table is non-decreasing from end to end.  Lane l
// makes group l (32 contiguous bytes of the slot, the maximum inside the lane, ONE scan over the lanes).
template <int LK>
__device__ __forceinline__ void bkt_bounds(const uint64_t *__restrict__ slot, uint32_t B, uint32_t *__restrict__ bnd, uint32_t lane)
{
    if constexpr (LK == kBktTwoLevel) {
        uint64_t *__restrict__ const tb = reinterpret_cast<uint64_t *>(bnd);
        unsigned long long v[kBktGroupSize];
#pragma unroll
        for (uint32_t c = 0; c < kBktGroupSize; ++c) {
            const uint32_t q = lane * kBktGroupSize + c;
            v[c] = slot[q < B ? q : 0u]; // (every lane loads, all four requests in flight before the first is looked at)
        }
        asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
        static_assert(kBktGroupSize == 4, "the four requests above");
#pragma unroll
        for (uint32_t c = 0; c < kBktGroupSize; ++c) {
            const uint32_t q = lane * kBktGroupSize + c;
            if (q == 0 || q >= B) v[c] = 0ull;
        }
#pragma unroll
        for (uint32_t c = 1; c < kBktGroupSize; ++c) v[c] = v[c] > v[c - 1] ? v[c] : v[c - 1];
        unsigned long long x = v[kBktGroupSize - 1]; // the group's maximum -> the maximum up to and with this group
#pragma unroll
        for (uint32_t m = 1; m < kWave; m <<= 1) {
            const unsigned long long y = __shfl_up(x, m);
            if (lane >= m && y > x) x = y;
        }
        unsigned long long before = __shfl_up(x, 1);
        if (lane == 0) before = 0ull;
#pragma unroll
        for (uint32_t c = 0; c < kBktGroupSize; ++c) {
            const uint32_t q = lane * kBktGroupSize + c;
            const unsigned long long m = v[c] > before ? v[c] : before;
            tb[bkt_slot_of(q)] = q == 0 ? 0ull : q < B ? spl_normalise(m) : ~0ull;
        }
    } else {
        constexpr uint32_t C = kBktMaxBuckets / kWave;
        unsigned long long v[C], carry = 0;
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) {
            const uint32_t q = c * kWave + lane;
            v[c] = q && q < B ? slot[q] : 0ull;
        }
#pragma unroll
        for (uint32_t c = 0; c < C; ++c) {
            unsigned long long x = v[c];
#pragma unroll
            for (uint32_t m = 1; m < kWave; m <<= 1) {
                const unsigned long long y = __shfl_up(x, m);
                if (lane >= m && y > x) x = y;
            }
            x = x > carry ? x : carry;
            carry = __shfl(x, kWave - 1);
            const uint32_t q = c * kWave + lane;
            const uint64_t t = q && q < B ? spl_normalise(x) : ~0ull;
            bnd[q] = (uint32_t)(t >> 32);
            bnd[kBktMaxBuckets + q] = (uint32_t)t;
        }
    }
}

// kBktTwoLevel: the last closed bound t_{B-1} (B >= 2), read ONCE by every wavefront behind the barrier into a
// wavefront-uniform pair: a key at or above it lies in the open bucket.  Both halves go through uint32_t:
// readfirstlane gives an int, and a sign-extended low half (a bound whose row-index word has its top bit set) would
// turn the bound into all-ones - no key open any more, and keys above every bound filed past the table.
// kBktFlat: nothing to read.
template <int LK>
__device__ __forceinline__ uint64_t bkt_last(const uint32_t *__restrict__ bnd, uint32_t B)
{
    if constexpr (LK == kBktTwoLevel) {
        const uint64_t t = reinterpret_cast<const uint64_t *>(bnd)[bkt_slot_of(B - 1u)];
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(t >> 32));
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)t);
        return ((uint64_t)hi << 32) | (uint64_t)lo;
    } else
        return 0ull;
}

// a key on its way into its bucket's list: key and segment (bucket * kSelListShards + shard) wavefront-uniform, pos lane
// 0's (the counter's answer)
struct BktPend {
    uint64_t key;
    uint32_t seg, pos;
};
constexpr uint32_t kBktNone = 0xFFFFFFFFu; // BktPend::seg: nothing on its way

// the store that a visit left behind: the counter has answered by now
__device__ __forceinline__ void bkt_flush(const SelLists &bk, const BktPend &pd, uint32_t lane)
{
    if (pd.seg != kBktNone && lane == 0 && pd.pos < kSelListSeg) bk.lists[(size_t)pd.seg * kSelListSeg + pd.pos] = pd.key;
}
// One wavefront-uniform key.  A CLOSED bucket (j < B - 1) counts the key in the caller's shard - every key, also beyond
// the segment's capacity - and the key is stored at the counter's answer by the NEXT visit (or bkt_flush): the answer
// then never stalls the caller's loop.  The open last bucket does nothing: it is P minus the closed ones, and while a
// run improves it is a third of the population.
// The count is an atomicInc that never wraps, not an atomicAdd: the compiler aggregates additions of a uniform value over
// the wavefront and WAITS for the answer on the spot (s_waitcnt vmcnt(0): the caller's rows in flight with it).
// kBktFlat: the full 64-bit compare against every bound (in a tie population the row index decides), a lane taking
// kBktMaxBuckets / 64 of them; the ballots' population counts add up to the bucket.  The fitness bits are compared
// first, and the row indices only where a bound has the key's fitness bits (wavefront-uniform).
// kBktTwoLevel (`last`: bkt_last): key >= last is the open bucket, with no LDS read and no ballot.  Otherwise lane l
// compares the key with the last bound of group l, the count is the number g of whole groups at or below the key
// (g < 64: the table's last bound is >= last > key); lanes 0 .. 3 compare it with the bounds of group g.  A key below
// t_{B-1} is in a closed bucket by construction.
template <int LK>
__device__ __forceinline__ void bkt_visit(const SelLists &bk, const uint32_t *__restrict__ bnd, uint64_t last, uint64_t key, uint32_t shard,
                                          uint32_t lane, BktPend &pd)
{
    bkt_flush(bk, pd, lane);
    if constexpr (LK == kBktTwoLevel) {
        pd.key = key;
        pd.seg = kBktNone;
        if (key >= last) return;
        const uint64_t *__restrict__ const tb = reinterpret_cast<const uint64_t *>(bnd);
        const uint32_t g = (uint32_t)__popcll(__ballot(tb[bkt_group_last(lane)] <= key));
        // (member c of group g: bkt_slot_of(4 g + c) = bkt_slot_of(c) + g; the lanes from 4 on re-read and are masked out)
        const uint32_t n = (uint32_t)__popcll(__ballot(tb[bkt_slot_of(lane & (kBktGroupSize - 1u)) + g] <= key) & ((1ull << kBktGroupSize) - 1ull));
        pd.seg = bkt_bucket_of(g, n) * kSelListShards + shard;
        if (lane == 0) pd.pos = atomicInc(&bk.cnt[pd.seg], 0xFFFFFFFFu);
    } else {
        const uint32_t kb = (uint32_t)(key >> 32), ki = (uint32_t)key;
        uint32_t j = 0;
        uint64_t ties[kBktMaxBuckets / kWave], any = 0;
#pragma unroll
        for (uint32_t c = 0; c < kBktMaxBuckets / kWave; ++c) {
            const uint32_t hi = bnd[c * kWave + lane];
            j += (uint32_t)__popcll(__ballot(hi < kb));
            ties[c] = __ballot(hi == kb);
            any |= ties[c];
        }
        if (any) {
#pragma unroll
            for (uint32_t c = 0; c < kBktMaxBuckets / kWave; ++c)
                j += (uint32_t)__popcll(ties[c] & __ballot(bnd[kBktMaxBuckets + c * kWave + lane] <= ki));
        }
        pd.key = key;
        pd.seg = j < bk.buckets - 1 ? j * kSelListShards + shard : kBktNone; // (buckets >= 2)
        if (pd.seg != kBktNone && lane == 0) pd.pos = atomicInc(&bk.cnt[pd.seg], 0xFFFFFFFFu);
    }
}

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
