// spectral_x.h -- rows of N = 256 and 2048 ... 8192 samples (1024 with -DSOTS_X_MIN=10), a wavefront per row and no LDS
// exchanges: k_fft_x with its x_* helpers, k_fitness_x (its stage-separated twin), and the kernels that lay out its tables
// (k_x_tables, k_x_seg_targets).
#pragma once
#include "common.h"
#include "fft.h"
#include "objective.h"
#include "stamps.h"

// contraction: on (the transform's mode, fft.h: k_fft_x<., 1> and k_fitness_x share their arithmetic with the helpers
// they call, and fused fitness equals staged fitness bit for bit only because both are compiled in one mode)
#pragma clang fp contract(on)
namespace sots { namespace {

// ------------------------------------------------------------------------------------
// Batched real FFT + fitness for N = 4096 (and 2048) WITHOUT LDS exchanges: one wavefront per row,
// E = N/128 complex points per lane in registers, the 64-point sub-transforms ACROSS lanes.
//
// The workgroup-per-row kernel that this one replaced made four dependent LDS round trips per row behind workgroup
// barriers, with 8 wavefronts per CU (0.40 of the HBM roofline at N = 4096).  Here a row never leaves
// the registers of its wavefront.  With M = 64 E complex points z[n], n = l + 64 j (lane l, register j):
//   Z[q + E p] = sum_l W_64^{l p} ( W_M^{l q} sum_j z[l + 64 j] W_E^{j q} )
//   1. an E-point DFT over j inside every lane (radix-2 DIF in registers; register r ends with q = bitrev(r));
//   2. the twiddle W_M^{l q};
//   3. for every register a 64-point DFT over the LANES: six radix-2 DIF stages whose partner lane is l ^ h,
//      h = 32, 16, 8, 4, 2, 1 - v_permlane32_swap, ds_swizzle (LDS crossbar, no LDS memory), DPP row rotate,
//      DPP quad permutes - a lane with bit h clear keeps a + b, the other one (a - b) W_2h^{l mod h}
//      (both as fma(own, +-1, partner) times a per-lane constant).  Lane l ends with p = bitrev6(l).
// So lane l, register r holds Z[k], k = bitrev(r) + E bitrev6(l): E consecutive bins per lane.  The real-input
// split needs Z[M - k]: register bitrev(E - q) of lane l ^ 63 (q >= 1) - one ds_bpermute per dword - and every
// lane turns E bins into squared errors: for half of its registers BOTH bins of the pair (k, M - k), its own and its
// partner lane's (round 4, pair2x: the pair's sum and twiddled difference are worked out once, not once in each of the two
// lanes).  Window, step-2 twiddles, split twiddles and target are laid out per (lane, register) in LDS once per workgroup
// (61 KiB, read as 16-byte words).
// ------------------------------------------------------------------------------------
constexpr int x_bitrev(int v, int bits)
{
    int r = 0;
    for (int i = 0; i < bits; ++i) r |= ((v >> i) & 1) << (bits - 1 - i);
    return r;
}
template <int LOG2N> constexpr int x_points() { return (1 << LOG2N) / 2 / kWave; }
// bits of a register index: log2 of a lane's E points
constexpr int x_point_bits(int e) { return e == 2 ? 1 : e == 4 ? 2 : e == 8 ? 3 : e == 16 ? 4 : e == 32 ? 5 : 6; }
#ifndef SOTS_X_WAVES12
#define SOTS_X_WAVES12 16
#endif
// wavefronts (independent rows) per workgroup: what the registers allow (MODE 0, the spectrum writer of the stage-separated
// path, needs a few more than the fused kernel)
template <int LOG2N, int MODE = 1> constexpr int x_waves() { return LOG2N >= 13 ? 8 : LOG2N == 12 ? (MODE == 0 ? 12 : SOTS_X_WAVES12) : 16; }
template <int LOG2N> constexpr bool x_applies() { return LOG2N >= 10 && LOG2N <= 13; }

// target bin of entry (lane l, register r) of k_fft_x's target table.  A lane turns out its own bin
// for the first register of a pair (RR, R2 = bitrev(E - bitrev(RR))) and its PARTNER lane's bin M - k for the second, so the
// second register's entry holds that bin's target: the partner is lane l ^ 63 (p' = 63 - p), its bin at r is q + E (63 - p).
template <int E, int EB>
__device__ __forceinline__ uint32_t x_target_bin(uint32_t l, uint32_t r)
{
    const uint32_t q = __brev(r) >> (32 - EB), pp = __brev(l) >> 26;
    const uint32_t r2 = q == 0 ? 0u : __brev((uint32_t)E - q) >> (32 - EB);
    return r2 < r ? q + E * (63u - pp) : q + E * pp;
}

// Complex values are 2-vectors here (register pairs): the transform is VALU-bound (85 % busy at 2400 one-float
// instructions per row in its first form), and v_pk_add/mul/fma_f32 do a complex add, or half a complex multiply, per
// instruction.
__device__ __forceinline__ v2f_t x_row_load(const float2 *p)
{
    return __builtin_nontemporal_load(reinterpret_cast<const v2f_t *>(p)); // rows are read once
}
// one radix-2 DIF stage of the E-point transform over the registers: pairs (a, a + H) inside groups of 2 H
template <int H, int E, int N>
__device__ __forceinline__ void x_reg_stage(v2f_t (&x)[E], const float2 *__restrict__ tw)
{
    static_for<0, E / 2>([&](auto i_tag) {
        constexpr int I = decltype(i_tag)::value, A0 = (I / H) * 2 * H, A = A0 + I % H;
        constexpr int IDX = (A - A0) * (E / (2 * H)); // the twiddle is W_E^IDX
        const v2f_t u = x[A] + x[A + H], d = x[A] - x[A + H];
        x[A] = u;
        if constexpr (IDX == 0) x[A + H] = d;
        else if constexpr (IDX == E / 4) x[A + H] = xc_mul_neg_i(d);
        else x[A + H] = xc_mul(d, xv(tw[IDX * (N / E)]));
    });
    if constexpr (H > 1) x_reg_stage<H / 2, E, N>(x, tw);
}


// one radix-2 DIF stage over the lanes, partner l ^ H, on every register: own * (+-1) + partner, times the lane's
// constant (1 where bit H is clear)
template <uint32_t H, int E>
__device__ __forceinline__ void x_lane_stage(v2f_t (&x)[E], float sgn, v2f_t wl)
{
#pragma unroll
    for (int r = 0; r < E; ++r) {
        const v2f_t p = v2f_t{lane_xor_f<H>(x[r].x), lane_xor_f<H>(x[r].y)};
        if constexpr (H != 1) { // the butterfly and its twiddle as one statement (see xc_mul)
            v2f_t t, u = x[r];
            asm("v_pk_fma_f32 %0, %0, %2, %3\n\t"
                "v_pk_mul_f32 %1, %0, %4 op_sel:[0,0] op_sel_hi:[1,0]\n\t"
                "v_pk_fma_f32 %0, %0, %4, %1 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]"
                : "+v"(u), "=&v"(t) : "v"(v2f_t{sgn, sgn}), "v"(p), "v"(wl));
            x[r] = u;
        } else {
            x[r] = x[r] * v2f_t{sgn, sgn} + p; // (the last stage's twiddle is 1)
        }
        if (r % 4 == 3) __builtin_amdgcn_sched_barrier(0); // (four registers' partner fetches in flight at a time)
    }
}

// The stages with partner l ^ 32 and l ^ 16 take the registers two at a time: v_permlane32_swap / v_permlane16_swap
// (new in gfx950) exchange the upper half (odd rows of 16) of one register with the lower half (even rows) of the other, so
// after swapping A with B the lanes with bit H clear hold BOTH inputs of register A's butterfly and the others both
// inputs of B's; every lane computes one whole butterfly (sum, difference times W_2H^{l mod H}) and a second pair of
// swaps puts the results where they belong.  Four swaps and four packed operations per pair of complex values, no
// per-lane signs, no select.
template <uint32_t H>
__device__ __forceinline__ void x_swap2(v2f_t &a, v2f_t &b)
{
    if constexpr (H == 32) {
        const auto r0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(a.x), __float_as_uint(b.x), false, false);
        const auto r1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(a.y), __float_as_uint(b.y), false, false);
        a = v2f_t{__uint_as_float(r0[0]), __uint_as_float(r1[0])}, b = v2f_t{__uint_as_float(r0[1]), __uint_as_float(r1[1])};
    } else {
        const auto r0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(a.x), __float_as_uint(b.x), false, false);
        const auto r1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(a.y), __float_as_uint(b.y), false, false);
        a = v2f_t{__uint_as_float(r0[0]), __uint_as_float(r1[0])}, b = v2f_t{__uint_as_float(r0[1]), __uint_as_float(r1[1])};
    }
}
template <uint32_t H, int E>
__device__ __forceinline__ void x_lane_stage_pairs(v2f_t (&x)[E], v2f_t w)
{
#pragma unroll
    for (int r = 0; r < E; r += 2) {
        x_swap2<H>(x[r], x[r + 1]);
        v2f_t sum = x[r] + x[r + 1], dif = xc_mul(x[r] - x[r + 1], w);
        x_swap2<H>(sum, dif);
        x[r] = sum, x[r + 1] = dif;
        if (r % 4 == 2) __builtin_amdgcn_sched_barrier(0);
    }
}

// WG: wavefronts per workgroup.  The default fills a CU with one workgroup (the tables are made once per workgroup); a SMALL
// population - fewer such workgroups than CUs - runs workgroups of four instead, a wavefront per SIMD on four times as many
// CUs: a row is then transformed at a lone wavefront's pace, not at a quarter of it (1024 rows of N = 4096: 24.6 -> ... us).
// floats of the per-(lane, register) tables as they lie in LDS: step-2 twiddles, split twiddles, window (float2 each), target
template <int LOG2N> constexpr int x_table_floats() { return 3 * 2 * kWave * (x_points<LOG2N>() + 2) + kWave * (x_points<LOG2N>() + 4); }

// `image` (fused kernel with window only; may be null): the four tables as they lie in LDS, made once per target by
// k_x_tables - the workgroups then copy them in by LDS-DMA, one round trip, instead of four dependent-index loads per entry
#ifndef SOTS_X_MIN_WAVES // (experiment: minimum wavefronts per SIMD the register allocation must allow, e.g. 5 with two workgroups of ten)
#define SOTS_X_MIN_WAVES 1
#endif
// floats of one chunk's target table in a segmented target image (SEG): the tgt_s part of the LDS tables, same layout
template <int LOG2N> constexpr uint32_t x_seg_stride() { return kWave * (x_points<LOG2N>() + 4); }
// SEG: as k_fft's - every row reads its chunk's target entries (lane, register) from the segmented image in global memory
// WGT: the weight table u in the layout of the target table (entry (l, r) at l (E + 4) + r: a one-chunk segmented image
// made from u[N/2]), read by (lane, register) from global memory - the LDS tables and their image stay as they are
template <int LOG2N, int MODE, bool WIN, int WG = x_waves<LOG2N, MODE>(), bool SEG = false, int OBJ = kObjMagnitude, bool WGT = false, typename... FLOOR>
__global__ __launch_bounds__((WG * kWave), (LOG2N == 12 && MODE == 1 ? SOTS_X_MIN_WAVES : 1)) void k_fft_x(const float *__restrict__ audio, float *__restrict__ spectrum,
                                                                   const float *__restrict__ target, float *__restrict__ fitness,
                                                                   const float2 *__restrict__ tw, const float *__restrict__ window,
                                                                   uint32_t p_len, float inv_n, float inv_wf, uint32_t pitch,
                                                                   const float *__restrict__ image, FLOOR... floor)
{
    static_assert(sizeof...(FLOOR) == (OBJ == kObjLogMagnitude ? 1 : 0) + (WGT ? 1 : 0) && ((OBJ == kObjMagnitude && !WGT) || MODE == 1), "the log instantiation (fitness epilogue only) takes the floor, the weighted one its table");
    static_assert(!WGT || WIN, "the weighted forms exist with a window only");
    [[maybe_unused]] const float floor_eps = trailing<float>(0.0f, floor...);
    [[maybe_unused]] const float *__restrict__ const wgt_u = trailing<const float *>(nullptr, floor...);
    constexpr int N = 1 << LOG2N, M = N / 2, E = x_points<LOG2N>(), EB = x_point_bits(E), W = WG;
    constexpr int S2 = E + 2, S1 = E + 4; // lane strides of the float2 / float tables (16-byte reads, spread over the banks)
    __shared__ __attribute__((aligned(16))) float xt_s[x_table_floats<LOG2N>()]; // (the variants without window or target leave theirs unused)
    float2 *const tw2_s = reinterpret_cast<float2 *>(xt_s), *const tws_s = tw2_s + kWave * S2, *const win_s = tws_s + kWave * S2;
    float *const tgt_s = reinterpret_cast<float *>(win_s + kWave * S2);
    __shared__ uint32_t next_s; // the workgroup's rows are dealt out as its wavefronts ask for them (below)
    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    if (tid == 0) next_s = W;
#ifdef SOTS_STAMP
    const unsigned long long xs_begin = __builtin_amdgcn_s_memrealtime(), xs_begin_clk = __builtin_amdgcn_s_memtime();
    unsigned long long xs_wait = 0, xs_rows = 0, xs_split = 0;
#endif
    if (MODE == 1 && WIN && image != nullptr) { // (launch_x_tables makes images only where the tables are whole 1 KiB pieces: N >= 2048)
        typedef __attribute__((address_space(3))) void *lds_ptr_t;
        for (uint32_t ch = wave; ch < (uint32_t)x_table_floats<LOG2N>() / 256u; ch += W)
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint32_t *>(image) + ch * 256u + lane * 4u, (lds_ptr_t)(xt_s + ch * 256u), 16, 0, 0);
        __builtin_amdgcn_s_waitcnt(0); // vmcnt(0): this wavefront's pieces have landed (the barrier below covers the others')
    } else
    for (uint32_t e = tid; e < kWave * E; e += W * kWave) {
        const uint32_t l = e / E, r = e % E;
        const uint32_t q = __brev(r) >> (32 - EB), pp = __brev(l) >> 26, k = q + E * pp;
        tw2_s[l * S2 + r] = tw[2u * l * q]; // W_M^{l q} = W_N^{2 l q}
        tws_s[l * S2 + r] = tw[k];          // W_N^k
        if constexpr (WIN) win_s[l * S2 + r] = reinterpret_cast<const float2 *>(window)[l + kWave * r]; // r = input register j here
        if constexpr (MODE == 1 && !SEG) tgt_s[l * S1 + r] = target[x_target_bin<E, EB>(l, r)];
    }
    const uint32_t seg_rows = SEG ? seg_target_rows(target) : 1u;
    // per-lane constants of the six lane stages
    const float sg8 = (lane & 8u) ? -1.0f : 1.0f;
    const float sg4 = (lane & 4u) ? -1.0f : 1.0f, sg2 = (lane & 2u) ? -1.0f : 1.0f, sg1 = (lane & 1u) ? -1.0f : 1.0f;
    const v2f_t one = v2f_t{1.0f, 0.0f};
    const v2f_t w32 = xv(tw[(lane & 31u) * (N / 64)]), w16 = xv(tw[(lane & 15u) * (N / 32)]); // (every lane makes a difference there)
    const v2f_t w8 = (lane & 8u) ? xv(tw[(lane & 7u) * (N / 16)]) : one, w4 = (lane & 4u) ? xv(tw[(lane & 3u) * (N / 8)]) : one;
    const v2f_t w2 = (lane & 2u) ? xv(tw[(lane & 1u) * (N / 4)]) : one;
    const uint32_t pp = __brev(lane) >> 26;
    const int addr_flip = (int)((lane ^ 63u) * 4u);                        // partner lane of the registers with q >= 1
    const int addr_zero = (int)((__brev((64u - pp) & 63u) >> 26) * 4u);    // ... and of register 0 (q = 0): Z[E (64 - p)]
    const float half_scale = 0.5f * (inv_n * inv_wf);
    __syncthreads();

    // Rows: workgroup b owns rows b W + w + i grid W (w < W, i = 0, 1, ...).  Its wavefronts start with i = 0, wavefront w
    // on row b W + w, and then take the workgroup's remaining rows in that order AS THEY FINISH: the SIMD issues for its
    // oldest wavefront first, so with a fixed deal of 8 rows each the wavefronts of one launch end anywhere between 77
    // and 148 us (N = 4096, P = 32768) and the last ones run alone, far below the issue rate (tools/fftx_probe.py).
    // Which wavefront transforms a row changes nothing in its result.
    uint32_t row = blockIdx.x * W + wave;
    if (row >= p_len) return;
#ifdef SOTS_STAMP
    const unsigned long long xs_tables = __builtin_amdgcn_s_memrealtime();
#endif
    v2f_t x[E];
    {
        const float2 *__restrict__ in = reinterpret_cast<const float2 *>(audio + (size_t)row * pitch);
#pragma unroll
        for (int j = 0; j < E; ++j) x[j] = x_row_load(in + lane + kWave * j);
    }
    while (true) {
        uint32_t take = 0;
        if (lane == 0) take = atomicAdd(&next_s, 1u); // (answered long before the split below needs it)
        take = __builtin_amdgcn_readfirstlane(take);
        const uint32_t nxt = blockIdx.x * W + take % W + (take / W) * gridDim.x * W;
        const bool more = nxt < p_len; // (rows past the end: every later take is past it too)
        __builtin_amdgcn_sched_barrier(0);
#ifdef SOTS_STAMP
        {
            const unsigned long long t0 = __builtin_amdgcn_s_memtime();
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            xs_wait += __builtin_amdgcn_s_memtime() - t0, xs_rows += 1;
        }
#endif
        if constexpr (WIN) {
#pragma unroll
            for (int j = 0; j < E; j += 2) {
                const float4 wv = *reinterpret_cast<const float4 *>(&win_s[lane * S2 + j]);
                x[j] = x[j] * v2f_t{wv.x, wv.y};
                x[j + 1] = x[j + 1] * v2f_t{wv.z, wv.w};
                if (j % 8 == 6) __builtin_amdgcn_sched_barrier(0); // (table reads a few at a time: the row already fills 2 E registers)
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // 1. E-point DIF over the registers
        x_reg_stage<E / 2, E, N>(x, tw);
        __builtin_amdgcn_sched_barrier(0);
        // 2. W_M^{l q}
#pragma unroll
        for (int r = 0; r < E; r += 2) {
            const float4 t = *reinterpret_cast<const float4 *>(&tw2_s[lane * S2 + r]);
            if (r) x[r] = xc_mul(x[r], v2f_t{t.x, t.y}); // register 0: q = 0
            x[r + 1] = xc_mul(x[r + 1], v2f_t{t.z, t.w});
            if (r % 8 == 6) __builtin_amdgcn_sched_barrier(0);
        }
        // 3. 64-point DIF over the lanes
        x_lane_stage_pairs<32>(x, w32);
        __builtin_amdgcn_sched_barrier(0);
        x_lane_stage_pairs<16>(x, w16);
        __builtin_amdgcn_sched_barrier(0);
        x_lane_stage<8>(x, sg8, w8);
        __builtin_amdgcn_sched_barrier(0);
        x_lane_stage<4>(x, sg4, w4);
        __builtin_amdgcn_sched_barrier(0);
        x_lane_stage<2>(x, sg2, w2);
        __builtin_amdgcn_sched_barrier(0);
        x_lane_stage<1>(x, sg1, one);
        __builtin_amdgcn_sched_barrier(0);
        // split: this lane's E bins k = bitrev(r) + E p
#ifdef SOTS_STAMP
        const unsigned long long xs_t2 = __builtin_amdgcn_s_memtime();
#endif
        float acc = 0.0f;
        // one bin: register RR of this lane with its partner Z[M - k]
        auto bin2x = [&](auto r_tag) -> v2f_t {
            constexpr int RR = decltype(r_tag)::value, Q = x_bitrev(RR, EB), R2 = Q == 0 ? 0 : x_bitrev(E - Q, EB);
            const int addr = Q == 0 ? addr_zero : addr_flip;
            const v2f_t zm = v2f_t{__int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(x[R2].x))),
                                   __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(x[R2].y)))};
            const v2f_t w = xv(tws_s[lane * S2 + RR]);
            const v2f_t ee = xc_add_conj(x[RR], zm), dd = xc_sub_conj(x[RR], zm);
            return ee + xc_mul_negi_w(dd, w); // 2 X[k] = (Z[k] + conj Z[M-k]) + W_N^k (-i) (Z[k] - conj Z[M-k])
        };
        // BOTH bins of the pair (k, M - k) from this lane's Z[k] (register RR) and the partner lane's Z[M - k] (its register
        // R2): ee and t = W_N^k (-i) dd once, 2 X[k] = ee + t and 2 conj X[M - k] = ee - t.  The partner lane does the same with
        // ITS register RR and this lane's R2, so every lane still turns out E bins - half of them its partner's - with half
        // the exchanges and a packed subtraction in place of a second add / subtract / multiply chain.
        auto pair2x = [&](auto r_tag, v2f_t &xa, v2f_t &xb) {
            constexpr int RR = decltype(r_tag)::value, Q = x_bitrev(RR, EB), R2 = x_bitrev(E - Q, EB);
            static_assert(Q != 0 && R2 != RR, "registers 0 and bitrev(E / 2) pair with themselves: bin2x");
            const v2f_t zm = v2f_t{__int_as_float(__builtin_amdgcn_ds_bpermute(addr_flip, __float_as_int(x[R2].x))),
                                   __int_as_float(__builtin_amdgcn_ds_bpermute(addr_flip, __float_as_int(x[R2].y)))};
            const v2f_t w = xv(tws_s[lane * S2 + RR]);
            const v2f_t ee = xc_add_conj(x[RR], zm), t = xc_mul_negi_w(xc_sub_conj(x[RR], zm), w);
            xa = ee + t, xb = ee - t;
        };
        if constexpr (MODE == 1) {
            // target entry (this lane, register RR): the workgroup's table in LDS, or (SEG) the row's chunk's in global memory
            const float *__restrict__ tg = SEG ? seg_target_chunk(target, row / seg_rows, x_seg_stride<LOG2N>()) + lane * S1 : nullptr;
            auto tgt_at = [&](int rr) -> float {
                if constexpr (SEG) return tg[rr];
                else return tgt_s[lane * S1 + rr];
            };
            [[maybe_unused]] const float *__restrict__ ul = WGT ? wgt_u + lane * S1 : nullptr;
            [[maybe_unused]] auto u_at = [&](int rr) -> float {
                if constexpr (WGT) return ul[rr];
                else return 0.0f;
            };
            // Registers RR and R2 = bitrev(E - bitrev(RR)) need each other and nobody else: the bins are taken in such
            // pairs (this is the summation order, k_fitness_x repeats it), and a pair that is done is free - the NEXT
            // row's loads into those two registers go out at once, so by the end of the split most of the next row is on
            // its way without a second set of registers.
            // (a wavefront's last row has no successor: it re-reads row 0, which every wavefront of the launch then finds in
            // L2 - loads under `if (more)` cost the compiler its register allocation)
            // the next row's address as a uniform base (scalar registers: audio + row offset) plus the lane's byte offset, instead
            // of the loop-invariant 64-bit pointer audio + lane offset plus a uniform row offset: with the pair split that pointer
            // was the one value too many for the 128 registers (an 8-byte spill, reloaded once per row; 130 against 127 us)
            // (the builtin returns a SIGNED int - the halves are widened as unsigned: the first attempt sign-extended the low
            // half and faulted on rows whose address has bit 31 set)
            const uint64_t in_next_u = reinterpret_cast<uint64_t>(audio + (size_t)(more ? nxt : 0u) * pitch);
            const uint32_t in_next_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)in_next_u);
            const uint32_t in_next_hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(in_next_u >> 32));
            typedef const __attribute__((address_space(1))) char *x_gptr_t; // global, not generic: global_load, not flat_load
            const x_gptr_t in_next_base = (x_gptr_t)(((uint64_t)in_next_hi << 32) | (uint64_t)in_next_lo);
            const uint32_t lane_bytes = lane * 8u;
            static_for<0, E>([&](auto r_tag) {
                constexpr int RR = decltype(r_tag)::value, Q = x_bitrev(RR, EB), R2 = Q == 0 ? 0 : x_bitrev(E - Q, EB);
                if constexpr (R2 >= RR) {
                    if constexpr (R2 != RR) {
                        v2f_t xa, xb;
                        pair2x(ic<RR>{}, xa, xb);
                        acc += bin_error<OBJ, WGT>(make_float2(xa.x, xa.y), tgt_at(RR), half_scale, floor_eps, u_at(RR));
                        acc += bin_error<OBJ, WGT>(make_float2(xb.x, xb.y), tgt_at(R2), half_scale, floor_eps, u_at(R2)); // the partner lane's bin M - k: x_target_bin
                    } else {
                        const v2f_t xa = bin2x(ic<RR>{});
                        acc += bin_error<OBJ, WGT>(make_float2(xa.x, xa.y), tgt_at(RR), half_scale, floor_eps, u_at(RR));
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    typedef const __attribute__((address_space(1))) v2f_t *x_gv2_t;
                    x[RR] = __builtin_nontemporal_load((x_gv2_t)(in_next_base + (lane_bytes + 8u * kWave * RR)));
                    if constexpr (R2 != RR) x[R2] = __builtin_nontemporal_load((x_gv2_t)(in_next_base + (lane_bytes + 8u * kWave * R2)));
                    __builtin_amdgcn_sched_barrier(0);
                }
            });
        } else
        static_for<0, E>([&](auto r_tag) { // MODE 0, the fused kernel's pairs: the same values, written where they belong
            constexpr int RR = decltype(r_tag)::value, Q = x_bitrev(RR, EB), R2 = Q == 0 ? 0 : x_bitrev(E - Q, EB);
            if constexpr (R2 >= RR) {
                float2 *__restrict__ bins = reinterpret_cast<float2 *>(spectrum + (size_t)row * (N + 8));
                const uint32_t k = E * pp + Q;
                if constexpr (R2 != RR) {
                    v2f_t xa, xb;
                    pair2x(ic<RR>{}, xa, xb);
                    bins[k] = make_float2(0.5f * xa.x, 0.5f * xa.y);
                    bins[M - k] = make_float2(0.5f * xb.x, -0.5f * xb.y);
                } else {
                    const v2f_t xa = bin2x(ic<RR>{});
                    bins[k] = make_float2(0.5f * xa.x, 0.5f * xa.y);
                }
            }
            if constexpr (RR % 4 == 3) __builtin_amdgcn_sched_barrier(0);
        });
        if constexpr (MODE == 0) {
            // the Nyquist bin X[M] = Re Z0 - Im Z0, from Z0 itself: lane 0 still holds it in register 0
            if (lane == 0) reinterpret_cast<float2 *>(spectrum + (size_t)row * (N + 8))[M] = make_float2(x[0].x - x[0].y, 0.0f);
        } else {
            acc = wave_sum(acc);
            if (lane == 0) fitness[row] = acc;
        }
#ifdef SOTS_STAMP
        xs_split += __builtin_amdgcn_s_memtime() - xs_t2;
        if (lane == 0 && blockIdx.x * W + wave < 2048) { // per wavefront: 8 words
            unsigned long long *o = g_stamps + (blockIdx.x * W + wave) * 8;
            o[0] = xs_begin, o[1] = xs_tables, o[2] = __builtin_amdgcn_s_memrealtime(), o[3] = xs_rows;
            o[4] = xs_wait, o[5] = xs_split, o[6] = __builtin_amdgcn_s_memtime() - xs_begin_clk;
        }
#endif
        if (!more) break;
        if constexpr (MODE == 0) { // (MODE 1 has asked for the row already, pair by pair)
            const float2 *__restrict__ in = reinterpret_cast<const float2 *>(audio + (size_t)nxt * pitch);
            static_for<0, E>([&](auto j_tag) { x[decltype(j_tag)::value] = x_row_load(in + lane + kWave * decltype(j_tag)::value); });
        }
        row = nxt;
    }
}

// fitnessPopulation on materialised rows with k_fft_x's bin -> (lane, register) map and summation order
template <int LOG2N, int OBJ = kObjMagnitude, bool WGT = false, typename... FLOOR>
__global__ __launch_bounds__(x_waves<LOG2N>() * kWave) void k_fitness_x(const float *__restrict__ spectrum, const float *__restrict__ target,
                                                                       float *__restrict__ fitness, uint32_t p_len, float inv_n, float inv_wf, FLOOR... floor)
{
    static_assert(sizeof...(FLOOR) == (OBJ == kObjLogMagnitude ? 1 : 0) + (WGT ? 1 : 0), "the log instantiation takes the floor, the weighted one its table");
    [[maybe_unused]] const float floor_eps = trailing<float>(0.0f, floor...);
    [[maybe_unused]] const float *__restrict__ const wgt_u = trailing<const float *>(nullptr, floor...);
    constexpr int N = 1 << LOG2N, E = x_points<LOG2N>(), EB = x_point_bits(E), W = x_waves<LOG2N>();
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t pp = __brev(lane) >> 26;
    for (uint32_t row = blockIdx.x * W + wave; row < p_len; row += gridDim.x * W) {
        const float2 *__restrict__ src = reinterpret_cast<const float2 *>(spectrum + (size_t)row * (N + 8)) + E * pp;
        float acc = 0.0f;
        if constexpr (WGT) {
            // The same pairs in the same order, as a loop: unrolled like the form below, the compiler reads row, target and
            // weights of all E registers ahead, and the third set of E registers spilled at N = 4096 and 8192.
            const float2 *__restrict__ bins = reinterpret_cast<const float2 *>(spectrum + (size_t)row * (N + 8));
#pragma unroll 2
            for (int rr = 0; rr < E; ++rr) {
                const int q = x_bitrev(rr, EB), r2 = q == 0 ? 0 : x_bitrev(E - q, EB);
                if (r2 < rr) continue;
                const int k = E * pp + q;
                acc += bin_error<OBJ, true>(bins[k], target[k], inv_n * inv_wf, floor_eps, wgt_u[k]);
                if (r2 != rr) {
                    const int k2 = N / 2 - k;
                    acc += bin_error<OBJ, true>(bins[k2], target[k2], inv_n * inv_wf, floor_eps, wgt_u[k2]);
                }
            }
        } else
        static_for<0, E>([&](auto r_tag) { // k_fft_x's order: register pairs (RR, R2 = bitrev(E - bitrev(RR)))
            constexpr int RR = decltype(r_tag)::value, Q = x_bitrev(RR, EB), R2 = Q == 0 ? 0 : x_bitrev(E - Q, EB);
            if constexpr (R2 >= RR) {
                acc += bin_error<OBJ, WGT>(src[Q], target[E * pp + Q], inv_n * inv_wf, floor_eps, WGT ? wgt_u[E * pp + Q] : 0.0f);
                // the pair's second bin is the PARTNER lane's: M - k (k_fft_x's pair2x)
                if constexpr (R2 != RR)
                    acc += bin_error<OBJ, WGT>(reinterpret_cast<const float2 *>(spectrum + (size_t)row * (N + 8))[N / 2 - (E * pp + Q)], target[N / 2 - (E * pp + Q)], inv_n * inv_wf, floor_eps, WGT ? wgt_u[N / 2 - (E * pp + Q)] : 0.0f);
            }
        });
        acc = wave_sum(acc);
        if (lane == 0) fitness[row] = acc;
    }
}
// the table image of the fused kernel (k_fft_x<LOG2N, 1, true>), entry by entry what its workgroups would make themselves
template <int LOG2N>
__global__ __launch_bounds__(256) void k_x_tables(float *__restrict__ image, const float2 *__restrict__ tw,
                                                  const float *__restrict__ window, const float *__restrict__ target)
{
    constexpr int E = x_points<LOG2N>(), EB = x_point_bits(E), S2 = E + 2, S1 = E + 4;
    float2 *const tw2_s = reinterpret_cast<float2 *>(image), *const tws_s = tw2_s + kWave * S2, *const win_s = tws_s + kWave * S2;
    float *const tgt_s = reinterpret_cast<float *>(win_s + kWave * S2);
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < (uint32_t)(kWave * E); e += gridDim.x * blockDim.x) {
        const uint32_t l = e / E, r = e % E;
        const uint32_t q = __brev(r) >> (32 - EB), pp = __brev(l) >> 26, k = q + E * pp;
        tw2_s[l * S2 + r] = tw[2u * l * q];
        tws_s[l * S2 + r] = tw[k];
        win_s[l * S2 + r] = reinterpret_cast<const float2 *>(window)[l + kWave * r];
        tgt_s[l * S1 + r] = target[x_target_bin<E, EB>(l, r)];
    }
}
// the target part of those tables for every chunk (segmented target image of k_fft_x<.., SEG>): chunk c's table from
// targets[c][N/2], entry (l, r) at l (E + 4) + r as in tgt_s (the padding entries stay as the caller left them)
// (one chunk's table, entry le = l E + r of its kWave E entries: the one copy both writers use - k_x_seg_targets for every chunk of a
// batch, the chunk queue's turnover for the slot it refills)
template <int LOG2N>
__device__ __forceinline__ void x_seg_target_entry(float *__restrict__ table, const float *__restrict__ target, uint32_t le)
{
    constexpr int E = x_points<LOG2N>(), EB = x_point_bits(E), S1 = E + 4;
    const uint32_t l = le / E, r = le % E;
    table[l * S1 + r] = target[x_target_bin<E, EB>(l, r)];
}
template <int LOG2N>
__global__ __launch_bounds__(256) void k_x_seg_targets(float *__restrict__ tables, const float *__restrict__ targets, uint32_t chunks)
{
    constexpr int E = x_points<LOG2N>();
    constexpr uint32_t M = (1u << LOG2N) / 2;
    const uint32_t total = chunks * (uint32_t)(kWave * E);
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t c = e / (kWave * E), le = e - c * (kWave * E);
        x_seg_target_entry<LOG2N>(tables + (size_t)c * x_seg_stride<LOG2N>(), targets + (size_t)c * M, le);
    }
}

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
