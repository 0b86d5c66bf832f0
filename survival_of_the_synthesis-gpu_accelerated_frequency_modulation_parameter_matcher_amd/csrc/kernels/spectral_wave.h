// spectral_wave.h -- rows of N <= 1024 samples, a wavefront per row: k_fft (Stockham passes through LDS, spectrum or fused
// fitness, optionally filing every row's selection key) and k_fitness, its stage-separated twin.
#pragma once
#include "common.h"
#include "fft.h"
#include "objective.h"
#include "sel_keys.h"
#include "stamps.h"

// contraction: on (the transform's mode, fft.h: k_fft<., 1> and k_fitness share their arithmetic with the helpers they
// call, and fused fitness equals staged fitness bit for bit only because both are compiled in one mode)
#pragma clang fp contract(on)
namespace sots { namespace {

// MODE 0: write spectrum rows; MODE 1: accumulate the fitness directly
// WIN: multiply by the fp32 window while loading (the generation loop then skips the window
// pass; the product is the same single fp32 rounding either way).
// Rows of N <= 1024 only (longer rows: k_fft_x).
// W: wavefronts per workgroup, each transforming rows of its own.  W = 1: workgroup b takes rows b, b + grid, ... - small
// populations, a wavefront wherever there is room.  W = 12 (N = 1024: what the registers let a CU hold, ONE workgroup per
// CU): the workgroup's rows b + t grid are dealt to its wavefronts as they ask (an LDS counter; every grid-th row, so that
// the whole GPU reads one moving window of the audio: a contiguous block of rows per workgroup is 8 % slower).  The SIMD issues for its
// oldest wavefront first: with a fixed deal the three wavefronts of a SIMD finish their equal shares one after the
// other and the last one runs alone, far below the issue rate (k_fft_x, kernels/spectral_x.h, has the numbers).
// SEG (chunks in flight, sots_batch): the rows belong to consecutive chunks of equal size, each with a target of its own;
// `target` is then a segmented target image (seg_target_rows / seg_target_chunk, kernels/objective.h) and every row reads its chunk's bins
// from it in global memory (L2) instead of the workgroup's one target in LDS.  Same arithmetic, same order.
template <int LOG2N> constexpr int fft_wide_waves() { return LOG2N == 10 ? 12 : 16; }
// The lists are one more kernel argument of the BUCKET instantiation ONLY (the first of the trailing arguments, kernels/objective.h):
// the others keep their argument list, and with it their code, to the byte (an argument in front of the hidden ones moves those).
struct BktNoLists {};
// BUCKET (the wide fitness kernel in front of a one-launch selection, list mode): every row's key goes into the list of
// its bucket between the splitters of bk.slot (bkt_visit, kernels/sel_keys.h) - the slot was written a generation ago, the row's
// fitness is in a register here, and the selection's 256 workgroups no longer ask all P rows each.
// OBJ (MODE 1): the objective; the log instantiations take the floor as their last argument (bin_error, kernels/objective.h)
// WGT (MODE 1): per-bin weights; the table u[N/2] is then the very last argument (bin_error2, kernels/objective.h).  Without SEG it sits
// in LDS beside the target, one float2 {target, u} per bin; with SEG the chunk's target is read from global memory as
// ever and u - one table for all chunks - sits in LDS on its own (read from global memory beside the target, the
// one-wavefront form needed 188 registers and lost its third wavefront per SIMD).
template <int LOG2N, int MODE, bool WIN, int W = 1, bool SEG = false, bool BUCKET = false, int OBJ = kObjMagnitude, bool WGT = false, typename... LISTS>
__global__ __launch_bounds__(W *kWave) void k_fft(const float *__restrict__ audio, float *__restrict__ spectrum,
                                                   const float *__restrict__ target, float *__restrict__ fitness,
                                                   const float2 *__restrict__ tw, const float *__restrict__ window,
                                                   uint32_t p_len, float inv_n, float inv_wf, uint32_t pitch, LISTS... lists)
{
    static_assert(sizeof...(LISTS) == (BUCKET ? 1 : 0) + (OBJ == kObjLogMagnitude ? 1 : 0) + (WGT ? 1 : 0), "the BUCKET instantiation takes the lists, the log ones the floor, the weighted ones their table, the others nothing");
    static_assert((OBJ == kObjMagnitude && !WGT) || MODE == 1, "the objective belongs to the fitness epilogue");
    static_assert(!WGT || WIN, "the weighted forms exist with a window only");
    using Lists = typename bkt_lists_of<LISTS...>::type; // (SelLists or SelListsTwoLevel: the lookup travels in the type)
    constexpr int LK = bkt_lookup_of<Lists>;
    [[maybe_unused]] const auto bk = trailing<Lists>(BktNoLists{}, lists...);
    [[maybe_unused]] const float floor_eps = trailing<float>(0.0f, lists...);
    [[maybe_unused]] const float *__restrict__ const wgt_u = trailing<const float *>(nullptr, lists...);
    constexpr int N = 1 << LOG2N, M = N / 2, E = M / kWave, H = E / 2;
    static_assert(LOG2N == 9 || LOG2N == 10, "wavefront-per-row FFT is for N <= 1024");
    static_assert(!BUCKET || (MODE == 1 && W > 1 && !SEG), "keys are filed by the wide fitness kernel only");
    __shared__ __attribute__((aligned(8))) uint32_t bnd_s[BUCKET ? 2 * kBktMaxBuckets : 1]; // (kBktTwoLevel reads whole keys)
    __shared__ float2 lds_all[W][M + M / 8 + 1];
    __shared__ uint32_t next_s;
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    float2 *const lds = lds_all[wave];
    const float half_scale = 0.5f * (inv_n * inv_wf); // the split below leaves a factor of two in
    const int partner_addr = ((kWave - lane) & (kWave - 1)) * 4; // ds_bpermute byte address of lane 64-l
    // buffer b0 starts with take `wave`, b1 with take W + wave; take t is row blockIdx.x + t grid
    const uint32_t grid = gridDim.x;
    uint32_t ind = blockIdx.x + wave * grid;
    if (W == 1 && ind >= p_len) return;
    // Three row buffers rotate (no copies): two rows are in flight beside the one being
    // transformed - a row's transform is shorter than the loaded memory latency, and the registers
    // are there (168 = three wavefronts per SIMD).
    constexpr int Q = E / 2; // rows are read 16 bytes per lane: pair index lane + 64 h holds complex points 2(lane+64h), +1
    auto request = [&](float4 (&dst)[Q], uint32_t r) { // rows past the end re-read the current one
        const float4 *__restrict__ in = reinterpret_cast<const float4 *>(audio + (size_t)(r < p_len ? r : ind) * pitch);
#pragma unroll
        for (int h = 0; h < Q; ++h) dst[h] = SOTS_ROW_LOAD(in + lane + kWave * h);
    };
    // The first two rows are asked for BEFORE the tables below: they need nothing but ind, p_len and pitch, and the
    // memory side then moves rows while the tables arrive.  What this buys is limited: loads return in order, so the
    // wait of the target's copy into LDS in front of the barrier (vmcnt(0)) now also waits for both rows - the barrier
    // stands behind the row latency instead of the row requests behind the barrier - and window and twiddles are still a
    // round trip of their own behind it.  Every table load stands behind the requests in the queue and is used before
    // the first row is, so the loop's waits still count row loads only.  A wavefront whose first row lies past the end
    // returns behind the barrier with two requests in flight: harmless, they read the workgroup's own first row
    // (blockIdx.x < p_len: no more workgroups than rows).
    float4 b0[Q], b1[Q], b2[Q];
    uint32_t r0 = ind, r1 = blockIdx.x + (W + wave) * grid, r2; // the rows in the three buffers
    const uint32_t first = ind < p_len ? ind : blockIdx.x;
    request(b0, first);
    asm volatile("" ::: "memory"); // keep the two requests in this order (the loop's waits count on it)
    request(b1, r1 < p_len ? r1 : first);
    asm volatile("" ::: "memory"); // ... and the tables behind them
    if (threadIdx.x == 0) next_s = 2 * W;

    // per-lane constants of the split / fitness step, loaded once (nothing but the audio
    // prefetch is in flight inside the loop, so its waits never drain the prefetch)
    float2 w_split[H];
#pragma unroll
    for (int q = 0; q < H; ++q) w_split[q] = tw[lane + kWave * q];
    // the target spectrum sits in LDS (2N bytes): eight registers fewer than holding this lane's
    // bins, which is what keeps N = 1024 at three wavefronts per SIMD with two rows in flight
    __shared__ float tgt_s[MODE == 1 && !SEG && !WGT ? M + 1 : 1];
    __shared__ float2 tu_s[MODE == 1 && !SEG && WGT ? M + 1 : 1]; // (weighted: {target, u} of a bin in one 8-byte read)
    __shared__ float u_s[MODE == 1 && SEG && WGT ? M + 1 : 1];
    if constexpr (MODE == 1 && SEG && WGT) {
        for (int k = threadIdx.x; k < M; k += W * kWave) u_s[k] = wgt_u[k];
    }
    if constexpr (MODE == 1 && !SEG && WGT) {
        for (int k = threadIdx.x; k < M; k += W * kWave) tu_s[k] = make_float2(target[k], wgt_u[k]);
    } else if constexpr (MODE == 1 && !SEG) {
        for (int k = threadIdx.x; k < M; k += W * kWave) tgt_s[k] = target[k];
    }
    const uint32_t seg_rows = SEG ? seg_target_rows(target) : 1u;
    if constexpr (BUCKET) {
        if (wave == W - 1) bkt_bounds<LK>(bk.slot, bk.buckets, bnd_s, lane); // (a wavefront of the workgroup's last rows)
    }
    if constexpr (MODE == 1 || W > 1) __syncthreads(); // (the only workgroup barrier: target, row counter and bounds are there)
    if (ind >= p_len) return;
    [[maybe_unused]] uint64_t bkt_end = 0ull; // the last closed bound, wavefront-uniform (kBktTwoLevel)
    if constexpr (BUCKET) bkt_end = bkt_last<LK>(bnd_s, bk.buckets);

    // (Window and twiddles stay BEHIND the barrier.  Asked for in front of it - pinned there, or the compiler sinks the
    // loads to their first use - they COST 0.5 us per generation, every round of eight.  Supposed, not shown: the slot
    // scan's loads and the target's copy then return behind 18 more loads per lane, and the barrier stands later.
    // profiles/r30_experiments.md)
    float4 wv[WIN ? Q : 1];
    if constexpr (WIN) {
#pragma unroll
        for (int h = 0; h < Q; ++h) wv[h] = reinterpret_cast<const float4 *>(window)[lane + kWave * h];
    }
    float2 twr[tw_count<M>()];
    preload_twiddles<M>(twr, tw, lane);
    // transforms the row in `cur` (individual `ind`) after requesting row ind + 2 grid into `fill`
#ifdef SOTS_STAMP
    unsigned long long st_wait = 0, st_fft = 0, st_tail = 0, st_rows = 0;
    const uint32_t st_slot = blockIdx.x * W + wave;
    const unsigned long long st_begin = __builtin_amdgcn_s_memrealtime(); // 100 MHz, common to the whole chip
    const unsigned long long st_begin_clk = __builtin_amdgcn_s_memtime();
#define SOTS_FFT_T(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#else
#define SOTS_FFT_T(var)
#endif
#ifdef SOTS_STAMP_ENDS
    // light stamps (no per-phase timers: the register allocation stays the product's): when every wavefront starts its
    // first row and ends, and how many rows it took (tools/fft_ends_probe.py)
    const unsigned long long se_begin = __builtin_amdgcn_s_memrealtime();
    uint32_t se_rows = 0;
#endif
    uint32_t pend = 0, dealt = 2; // the take on its way (lane 0) / W = 1: takes so far
    auto next_take = [&]() {
        if constexpr (W == 1) return dealt++;
        else {
            const uint32_t t = __builtin_amdgcn_readfirstlane(pend);
            if (lane == 0) pend = atomicAdd(&next_s, 1u); // answered during this row's transform
            return t;
        }
    };
    if constexpr (W > 1) {
        if (lane == 0) pend = atomicAdd(&next_s, 1u);
    }
    BktPend bkt = {0ull, kBktNone, 0u}; // the key whose place in its list is on its way (BUCKET)
    // transforms the row in `cur` (row `ind`) after requesting this wavefront's next take into `fill`; returns that row
    auto process = [&](float4 (&cur)[Q], float4 (&fill)[Q]) -> uint32_t {
        SOTS_FFT_T(t0);
#ifdef SOTS_STAMP
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(Q) : "memory"); // the row in `cur` has landed (the newer request may still fly)
#endif
        SOTS_FFT_T(t1);
        if constexpr (WIN) {
#pragma unroll
            for (int h = 0; h < Q; ++h) { // two packed multiplies per 16 bytes
                const v2f_t lo = v2f_t{cur[h].x, cur[h].y} * v2f_t{wv[h].x, wv[h].y}, hi = v2f_t{cur[h].z, cur[h].w} * v2f_t{wv[h].z, wv[h].w};
                cur[h] = make_float4(lo.x, lo.y, hi.x, hi.y);
            }
        }
        const uint32_t filled = blockIdx.x + next_take() * grid;
        request(fill, filled);
#ifdef SOTS_STAMP_ENDS
        ++se_rows;
#endif
        float2 z[E]; // z[s] = Z[lane + 64 s]
        fft_forward<M, W == 1>(cur, lds, tw, twr, lane, z);
        SOTS_FFT_T(t2);
        // bin M/2 = conj Z[M/2]; Z[M/2] = Z[0 + 64 (E/2)] is lane 0's slot E/2, and only lane 0 (k = 0) uses it
        const float2 x_half = make_float2(z[E / 2].x, -z[E / 2].y);
        if constexpr (MODE == 0) {
            float2 *__restrict__ row = reinterpret_cast<float2 *>(spectrum + (size_t)ind * (N + 8));
#pragma unroll
            for (int q = 0; q < H; ++q) {
                const int k = lane + kWave * q;
                v2f_t xa2, xbc2;
                split_pair_2x(z[q], split_partner<M>(z, q, lane, partner_addr), w_split[q], xa2, xbc2);
                row[k] = make_float2(0.5f * xa2.x, 0.5f * xa2.y);
                row[M - k] = make_float2(0.5f * xbc2.x, -0.5f * xbc2.y); // k = 0 lands on the Nyquist bin M
            }
            if (lane == 0) row[M / 2] = x_half;
        } else {
            v2f_t acc2 = v2f_t{0.0f, 0.0f};
            const float *__restrict__ tg = SEG ? seg_target_chunk(target, ind / seg_rows, M) : nullptr;
#pragma unroll
            for (int q = 0; q < H; ++q) {
                const int k = lane + kWave * q;
                v2f_t xa2, xbc2;
                split_pair_2x(z[q], split_partner<M>(z, q, lane, partner_addr), w_split[q], xa2, xbc2); // 2 X[k], 2 conj X[M-k]
                if (k == 0) xbc2 = v2f_t{2.0f * x_half.x, 2.0f * x_half.y}; // the fitness skips the Nyquist bin and needs bin M/2
                if constexpr (WGT) {
                    const int k2 = k == 0 ? M / 2 : M - k;
                    if constexpr (SEG) {
                        bin_error2<OBJ, true>(acc2, make_float2(xa2.x, xa2.y), make_float2(xbc2.x, xbc2.y), tg[k], tg[k2], half_scale, floor_eps, u_s[k], u_s[k2]);
                        if constexpr (W == 1) __builtin_amdgcn_sched_barrier(0); // (the one-wavefront form: read ahead, the weights cost the third wavefront per SIMD)
                    }
                    else {
                        const float2 ta = tu_s[k], tb = tu_s[k2];
                        bin_error2<OBJ, true>(acc2, make_float2(xa2.x, xa2.y), make_float2(xbc2.x, xbc2.y), ta.x, tb.x, half_scale, floor_eps, ta.y, tb.y);
                    }
                } else
                if constexpr (SEG) bin_error2<OBJ, false>(acc2, make_float2(xa2.x, xa2.y), make_float2(xbc2.x, xbc2.y), tg[k], tg[k == 0 ? M / 2 : M - k], half_scale, floor_eps, 0.0f, 0.0f);
                else bin_error2<OBJ, false>(acc2, make_float2(xa2.x, xa2.y), make_float2(xbc2.x, xbc2.y), tgt_s[k], tgt_s[k == 0 ? M / 2 : M - k], half_scale, floor_eps, 0.0f, 0.0f);
            }
            float acc = wave_sum(acc2.x + acc2.y);
            if (lane == 0) fitness[ind] = acc;
            if constexpr (BUCKET) {
                // (uniform by construction; said to the compiler so that key and bucket stay in scalar registers)
                const uint32_t kb = __builtin_amdgcn_readfirstlane(order_bits(acc));
                bkt_visit<LK>(bk, bnd_s, bkt_end, ((uint64_t)kb << 32) | ind, blockIdx.x % kSelListShards, lane, bkt);
            }
        }
        wave_lds_sync<W == 1>(); // orders this row's LDS reads before the next row's writes
#ifdef SOTS_STAMP
        {
            const unsigned long long t3 = __builtin_amdgcn_s_memtime();
            if (st_rows == 0 && lane == 0 && st_slot < 512) g_stamps[3 * 8192 + st_slot * 16 + 7] = t0 - st_begin_clk; // prologue
            st_wait += t1 - t0, st_fft += t2 - t1, st_tail += t3 - t2, st_rows += 1;
            if (lane == 0 && st_slot < 512) {
                g_stamps[3 * 8192 + st_slot * 16 + 0] = st_wait;
                g_stamps[3 * 8192 + st_slot * 16 + 1] = st_fft;
                g_stamps[3 * 8192 + st_slot * 16 + 2] = st_tail;
                g_stamps[3 * 8192 + st_slot * 16 + 3] = st_rows;
                g_stamps[3 * 8192 + st_slot * 16 + 4] = st_begin;
                g_stamps[3 * 8192 + st_slot * 16 + 5] = __builtin_amdgcn_s_memrealtime();
                g_stamps[3 * 8192 + st_slot * 16 + 6] = __builtin_amdgcn_s_memtime() - st_begin_clk;
            }
        }
#endif
        return filled;
    };
    while (true) { // (takes only grow: a wavefront whose next row is past the end has no later one either)
        ind = r0, r2 = process(b0, b2);
        if (r1 >= p_len) break;
        ind = r1, r0 = process(b1, b0);
        if (r2 >= p_len) break;
        ind = r2, r1 = process(b2, b1);
        if (r0 >= p_len) break;
    }
    if constexpr (BUCKET) bkt_flush(bk, bkt, lane);
#ifdef SOTS_STAMP_ENDS
    if (lane == 0 && blockIdx.x * W + wave < 4096) {
        unsigned long long *o = g_stamps + (blockIdx.x * W + wave) * 4;
        o[0] = se_begin, o[1] = __builtin_amdgcn_s_memrealtime(), o[2] = se_rows, o[3] = __builtin_amdgcn_s_getreg(4 | (0 << 6) | ((16 - 1) << 11)); // HW_ID: wave, SIMD, CU, SH, SE
    }
#endif
}

// fitnessPopulation on materialised spectrum rows; same bin -> lane assignment and
// summation order as k_fft<.., 1>, so both paths give the same fp32 sum.
template <int LOG2N, int OBJ = kObjMagnitude, bool WGT = false, typename... FLOOR>
__global__ __launch_bounds__(kWave) void k_fitness(const float *__restrict__ spectrum,
                                                   const float *__restrict__ target,
                                                   float *__restrict__ fitness, uint32_t p_len, float inv_n,
                                                   float inv_wf, FLOOR... floor)
{
    static_assert(sizeof...(FLOOR) == (OBJ == kObjLogMagnitude ? 1 : 0) + (WGT ? 1 : 0), "the log instantiation takes the floor, the weighted one its table");
    [[maybe_unused]] const float floor_eps = trailing<float>(0.0f, floor...);
    [[maybe_unused]] const float *__restrict__ const wgt_u = trailing<const float *>(nullptr, floor...);
    constexpr int N = 1 << LOG2N, M = N / 2, E = M / kWave;
    const int lane = threadIdx.x;
    for (uint32_t ind = blockIdx.x; ind < p_len; ind += gridDim.x) {
        const float2 *__restrict__ row = reinterpret_cast<const float2 *>(spectrum + (size_t)ind * (N + 8));
        v2f_t acc2 = v2f_t{0.0f, 0.0f};
#pragma unroll
        for (int q = 0; q < E / 2; ++q) {
            const int k = lane + kWave * q;
            const int kb = k == 0 ? M / 2 : M - k;
            bin_error2<OBJ, WGT>(acc2, row[k], row[kb], target[k], target[kb], inv_n * inv_wf, floor_eps, WGT ? wgt_u[k] : 0.0f, WGT ? wgt_u[kb] : 0.0f);
        }
        float acc = wave_sum(acc2.x + acc2.y);
        if (lane == 0) fitness[ind] = acc;
    }
}

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
