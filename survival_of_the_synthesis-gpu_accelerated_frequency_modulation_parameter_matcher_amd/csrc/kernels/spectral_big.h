// spectral_big.h -- rows of N = 16384 and 32768 samples, a workgroup per row with the points in LDS: k_fft_big and
// k_fitness_big, its stage-separated twin.
#pragma once
#include "common.h"
#include "fft.h"
#include "objective.h"

// contraction: on (the transform's mode, fft.h: k_fft_big<., 1> and k_fitness_big share their arithmetic with the
// helpers they call)
#pragma clang fp contract(on)
namespace sots { namespace {

// ------------------------------------------------------------------------------------
// Rows of N = 16384 and 32768 samples (round 4: the reference takes any audioLengthLog2, main.cpp:90, and renders 2^14
// samples of its best match, main.cpp:273): a WORKGROUP per row.  Such a row is 128 or 256 registers per lane of one
// wavefront, more than k_fft_x can hold; here its M = N / 2 complex points live in LDS (64 or 128 KiB), 512 threads run an
// in-place radix-2 DIF (natural order in, bit-reversed out) with one workgroup barrier per stage, and the real-input split
// reads Z[k] and Z[M - k] at their bit-reversed places.  Coverage, not speed: nothing of BASELINE's configs runs here.
//   MODE 0: spectrum row (bins 0 .. M) to memory; MODE 1: squared error against the target, bins 0 .. M-1
//   (Evolutionary_Strategy_CPU.hpp:235).  Thread t takes bins t, t + 512, ... in rising order, the wavefront totals are added
//   in wavefront order; k_fitness_big repeats map and order on a materialised row (bit-identical sums).
// ------------------------------------------------------------------------------------
constexpr int kBigThreads = 512;
template <int LOG2N> constexpr bool big_applies() { return LOG2N == 14 || LOG2N == 15; }

__device__ __forceinline__ float big_block_sum(float acc, float *__restrict__ red)
{
    acc = wave_sum(acc);
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    float total = 0.0f;
    if (threadIdx.x == 0)
        for (int w = 0; w < kBigThreads / kWave; ++w) total += red[w];
    return total; // (thread 0's)
}

// SEG: `target` is a segmented target image (k_fft's, kernels/spectral_wave.h); row r takes its chunk's bins
template <int LOG2N, int MODE, bool WIN, bool SEG = false, int OBJ = kObjMagnitude, bool WGT = false, typename... FLOOR>
__global__ __launch_bounds__(kBigThreads) void k_fft_big(const float *__restrict__ audio, float *__restrict__ spectrum,
                                                         const float *__restrict__ target, float *__restrict__ fitness,
                                                         const float2 *__restrict__ tw, const float *__restrict__ window,
                                                         uint32_t p_len, float inv_n, float inv_wf, uint32_t pitch, FLOOR... floor)
{
    static_assert(sizeof...(FLOOR) == (OBJ == kObjLogMagnitude ? 1 : 0) + (WGT ? 1 : 0) && ((OBJ == kObjMagnitude && !WGT) || MODE == 1), "the log instantiation (fitness epilogue only) takes the floor, the weighted one its table");
    static_assert(!WGT || WIN, "the weighted forms exist with a window only");
    [[maybe_unused]] const float floor_eps = trailing<float>(0.0f, floor...);
    [[maybe_unused]] const float *__restrict__ const wgt_u = trailing<const float *>(nullptr, floor...);
    constexpr uint32_t N = 1u << LOG2N, M = N / 2, LM = LOG2N - 1, T = kBigThreads;
    extern __shared__ float2 big_z[]; // M complex points (the launch asks for M * 8 + 64 bytes)
    float *__restrict__ red = reinterpret_cast<float *>(big_z + M);
    const uint32_t t = threadIdx.x;
    for (uint32_t row = blockIdx.x; row < p_len; row += gridDim.x) {
        const float2 *__restrict__ in = reinterpret_cast<const float2 *>(audio + (size_t)row * pitch);
        for (uint32_t i = t; i < M; i += T) {
            float2 v = in[i];
            if constexpr (WIN) {
                const float2 w = reinterpret_cast<const float2 *>(window)[i];
                v.x *= w.x, v.y *= w.y;
            }
            big_z[i] = v;
        }
        __syncthreads();
        // in-place radix-2 DIF: stage s pairs i and i + half, half = M >> (s + 1); the difference takes W_{2 half}^{j} = W_N^{j N / (2 half)}
        for (uint32_t st = 0; st < LM; ++st) {
            const uint32_t half = M >> (st + 1), tw_step = N / (2u * half);
            for (uint32_t b = t; b < M / 2; b += T) {
                const uint32_t j = b & (half - 1), i0 = ((b - j) << 1) + j, i1 = i0 + half;
                const float2 a = big_z[i0], c = big_z[i1];
                big_z[i0] = cadd(a, c);
                const float2 d = csub(a, c);
                big_z[i1] = j == 0 ? d : cmul(d, tw[j * tw_step]);
            }
            __syncthreads();
        }
        // Z[k] now lies at bitrev(k).  X[k] = (Z[k] + conj Z[M-k]) / 2 + W_N^k (-i) (Z[k] - conj Z[M-k]) / 2, Z[M] read as Z[0]
        auto bin = [&](uint32_t k) -> float2 {
            const uint32_t km = (M - k) & (M - 1);
            const float2 a = big_z[__brev(k) >> (32 - LM)], bz = big_z[__brev(km) >> (32 - LM)];
            const float2 ee = make_float2(0.5f * (a.x + bz.x), 0.5f * (a.y - bz.y)), dd = make_float2(0.5f * (a.x - bz.x), 0.5f * (a.y + bz.y));
            const float2 o = make_float2(dd.y, -dd.x); // -i dd
            const float2 w = tw[k];
            return make_float2(ee.x + (o.x * w.x - o.y * w.y), ee.y + (o.x * w.y + o.y * w.x));
        };
        if constexpr (MODE == 0) {
            float2 *__restrict__ dst = reinterpret_cast<float2 *>(spectrum + (size_t)row * (N + 8));
            for (uint32_t k = t; k < M; k += T) dst[k] = bin(k);
            if (t == 0) dst[M] = make_float2(big_z[0].x - big_z[0].y, 0.0f); // the Nyquist bin X[M] = Re Z0 - Im Z0
        } else {
            float acc = 0.0f;
            const float *__restrict__ tg = SEG ? seg_target_chunk(target, row / seg_target_rows(target), M) : target;
            for (uint32_t k = t; k < M; k += T) acc += bin_error<OBJ, WGT>(bin(k), tg[k], inv_n * inv_wf, floor_eps, WGT ? wgt_u[k] : 0.0f);
            const float total = big_block_sum(acc, red);
            if (t == 0) fitness[row] = total;
        }
        __syncthreads(); // the next row overwrites big_z and red
    }
}

template <int LOG2N, int OBJ = kObjMagnitude, bool WGT = false, typename... FLOOR>
__global__ __launch_bounds__(kBigThreads) void k_fitness_big(const float *__restrict__ spectrum, const float *__restrict__ target,
                                                             float *__restrict__ fitness, uint32_t p_len, float inv_n, float inv_wf, FLOOR... floor)
{
    static_assert(sizeof...(FLOOR) == (OBJ == kObjLogMagnitude ? 1 : 0) + (WGT ? 1 : 0), "the log instantiation takes the floor, the weighted one its table");
    [[maybe_unused]] const float floor_eps = trailing<float>(0.0f, floor...);
    [[maybe_unused]] const float *__restrict__ const wgt_u = trailing<const float *>(nullptr, floor...);
    constexpr uint32_t N = 1u << LOG2N, M = N / 2, T = kBigThreads;
    __shared__ float red[kBigThreads / kWave];
    for (uint32_t row = blockIdx.x; row < p_len; row += gridDim.x) {
        const float2 *__restrict__ src = reinterpret_cast<const float2 *>(spectrum + (size_t)row * (N + 8));
        float acc = 0.0f;
        for (uint32_t k = threadIdx.x; k < M; k += T) acc += bin_error<OBJ, WGT>(src[k], target[k], inv_n * inv_wf, floor_eps, WGT ? wgt_u[k] : 0.0f);
        const float total = big_block_sum(acc, red);
        if (threadIdx.x == 0) fitness[row] = total;
        __syncthreads();
    }
}

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
