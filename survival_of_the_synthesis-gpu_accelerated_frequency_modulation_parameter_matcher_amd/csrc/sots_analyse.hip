// sots_analyse.hip -- analysis on the device: k_analyse, the windowed real-input FFT of overlapping
// frames read in place from one buffer, and k_score_frames, the objective of such frames against stored targets.
//
// k_analyse: a workgroup per frame, the N/2 complex points z[i] = (w[2i] s[2i], w[2i+1] s[2i+1]) in LDS (1 KiB at N = 256,
// 128 KiB at N = 32768).  The transform is an in-place decimation in frequency: two radix-2 layers per trip through LDS
// (four points in registers, three table twiddles), one plain radix-2 layer at the end where log2(N/2) is odd, a
// workgroup barrier after each trip.  Z[k] then lies at the bit-reversed index of k; the real-input split reads Z[k] and
// Z[M - k] from there and stores bin k, so the stores are coalesced and the reversal costs no pass of its own.
// The samples are loaded one dword per lane per load: a frame starts at f * hop, any alignment, and the same instructions
// serve every hop - a frame's bits cannot depend on where it starts.  Overlapping frames re-read their samples from L2.
// No atomics, no scratch; the only memory written is the frame's own N/2 outputs.
#include "sots_analyse.h"

#include "kernels/fft.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function" // (k_objective_map: launched from sots_kernels.hip, not from here)
#include "kernels/objective.h"
#pragma clang diagnostic pop

namespace sots {

namespace {

#pragma clang fp contract(on) // (the mode of kernels/fft.h and of bin_error's magnitude)

// the magnitude exactly as bin_error takes it of the same bin: one expression, the same contraction
__device__ __forceinline__ float bin_magnitude(float2 x) { return __builtin_amdgcn_sqrtf(x.x * x.x + x.y * x.y); }

template <int LOG2N> constexpr int analyse_threads()
{
    constexpr int quads = (1 << LOG2N) / 8; // four-point butterflies of one trip
    return quads < 64 ? 64 : quads > 1024 ? 1024 : quads;
}

// The layers of block length L, L/2 (one trip: points base + {0, q, 2q, 3q}, q = L/4) and on down; L == 2: the last layer
// alone.  tw[i] = e^{-2 pi i / N} of the engine's table, N = 2 M, so W_L^j = tw[j (N / L)].
template <int M, int L, int T>
__device__ __forceinline__ void analyse_layers(float2 *__restrict__ lds, const float2 *__restrict__ tw, int t)
{
    if constexpr (L >= 4) {
        constexpr int q = L / 4, ts = (2 * M) / L;
        for (int g = t; g < M / 4; g += T) {
            const int j = g & (q - 1), base = ((g - j) << 2) + j;
            const float2 a0 = lds[base], a1 = lds[base + q], a2 = lds[base + 2 * q], a3 = lds[base + 3 * q];
            const float2 w1 = tw[j * ts], w1q = tw[(j + q) * ts], w2 = tw[2 * j * ts];
            // layer of length L: (a0, a2) at j, (a1, a3) at j + q
            const float2 b0 = cadd(a0, a2), b2 = cmul(csub(a0, a2), w1);
            const float2 b1 = cadd(a1, a3), b3 = cmul(csub(a1, a3), w1q);
            // layer of length L/2: (b0, b1) in the lower half, (b2, b3) in the upper, both at j
            lds[base] = cadd(b0, b1);
            lds[base + q] = cmul(csub(b0, b1), w2);
            lds[base + 2 * q] = cadd(b2, b3);
            lds[base + 3 * q] = cmul(csub(b2, b3), w2);
        }
        __syncthreads();
        analyse_layers<M, L / 4, T>(lds, tw, t);
    } else if constexpr (L == 2) {
        for (int g = t; g < M / 2; g += T) {
            const float2 a = lds[2 * g], b = lds[2 * g + 1];
            lds[2 * g] = cadd(a, b);
            lds[2 * g + 1] = csub(a, b);
        }
        __syncthreads();
    }
}

// BINS: out holds the scaled bins (float2) instead of their magnitudes
template <int LOG2N, bool BINS>
__global__ __launch_bounds__(analyse_threads<LOG2N>()) void k_analyse(const float *__restrict__ signal, const float *__restrict__ window,
                                                                      const float2 *__restrict__ tw, float *__restrict__ out, uint32_t hop,
                                                                      float scale_half)
{
    constexpr int M = (1 << LOG2N) / 2, T = analyse_threads<LOG2N>();
    extern __shared__ __attribute__((aligned(16))) unsigned char analyse_lds[];
    float2 *lds = reinterpret_cast<float2 *>(analyse_lds);
    const int t = (int)threadIdx.x;
    const float *s = signal + (size_t)blockIdx.x * hop; // the frame's N samples: s[0 .. 2 M)
    for (int i = t; i < M; i += T) {
        const float2 w = reinterpret_cast<const float2 *>(window)[i];
        lds[i] = make_float2(s[2 * i] * w.x, s[2 * i + 1] * w.y);
    }
    __syncthreads();
    analyse_layers<M, M, T>(lds, tw, t);

    // Real-input split (kernels/fft.h): 2 X[k] = (Z[k] + conj Z[M-k]) + e^{-2 pi i k / N} (-i) (Z[k] - conj Z[M-k]), Z[M] = Z[0].
    // The 2 goes into the scale (exact), and the scale onto the bin before its magnitude (sots_analyse.h).
    const size_t row = (size_t)blockIdx.x * M;
    for (int k = t; k < M; k += T) {
        const int ka = (int)(__brev((uint32_t)k) >> (33 - LOG2N));
        const int kb = (int)(__brev((uint32_t)((M - k) & (M - 1))) >> (33 - LOG2N));
        const float2 a = lds[ka], b = lds[kb];
        const float2 ee = make_float2(a.x + b.x, a.y - b.y), dd = make_float2(a.x - b.x, a.y + b.y);
        const float2 x2 = cadd(ee, cmul(make_float2(dd.y, -dd.x), tw[k]));
        const float2 x = make_float2(x2.x * scale_half, x2.y * scale_half);
        if constexpr (BINS) reinterpret_cast<float2 *>(out)[row + k] = x;
        else out[row + k] = bin_magnitude(x);
    }
}

// a wavefront per frame; the order of the sum is the header's
template <int OBJ, bool WGT>
__global__ __launch_bounds__(kWave) void k_score_frames(const float2 *__restrict__ bins, const float *__restrict__ targets,
                                                        const float *__restrict__ u, float *__restrict__ fitness, uint32_t m, float floor)
{
    const size_t row = (size_t)blockIdx.x * m;
    float acc = 0.0f;
    for (uint32_t k = threadIdx.x; k < m; k += kWave) {
        const float e2 = bin_error<OBJ, WGT>(bins[row + k], targets[row + k], 1.0f, floor, WGT ? u[k] : 1.0f);
        acc = acc + e2;
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) fitness[blockIdx.x] = acc;
}

#pragma clang fp contract(off)

template <int LOG2N, bool BINS>
hipError_t launch_analyse_as(hipStream_t st, const float *signal, const float *window, const float2 *twiddle, float *out, uint32_t hop,
                             uint32_t frames, float scale_half)
{
    const auto kernel = k_analyse<LOG2N, BINS>;
    const size_t lds = ((size_t)1 << LOG2N) / 2 * sizeof(float2);
    if (lds > 48u * 1024u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    kernel<<<frames, analyse_threads<LOG2N>(), lds, st>>>(signal, window, twiddle, out, hop, scale_half);
    return hipGetLastError();
}

template <int OBJ, bool WGT>
hipError_t launch_score_as(hipStream_t st, const float2 *bins, const float *targets, const float *u, float *fitness, uint32_t m, uint32_t frames,
                           float floor)
{
    k_score_frames<OBJ, WGT><<<frames, kWave, 0, st>>>(bins, targets, u, fitness, m, floor);
    return hipGetLastError();
}

hipError_t grow(float *&buf, size_t &have, size_t need)
{
    if (need <= have) return hipSuccess;
    if (buf) {
        const hipError_t e = hipFree(buf);
        buf = nullptr, have = 0;
        if (e != hipSuccess) return e;
    }
    const hipError_t e = hipMalloc((void **)&buf, need * sizeof(float));
    if (e != hipSuccess) return buf = nullptr, e;
    have = need;
    return hipSuccess;
}

} // namespace

hipError_t launch_analyse(hipStream_t st, const float *signal, const float *window, const float2 *twiddle, float *out, bool bins,
                          uint32_t log2n, uint32_t hop, uint32_t frames, float inv_n, float inv_wf)
{
    if (!signal || !window || !twiddle || !out || frames == 0 || log2n < 8 || log2n > 15 || hop == 0 || hop > (1u << log2n))
        return hipErrorInvalidValue;
    const float scale_half = inv_n * inv_wf * 0.5f; // (the fitness kernels' scale / 2: a power of two apart, the same bits)
#define SOTS_ANALYSE_CASE(L)                                                                                                   \
    case L:                                                                                                                    \
        return bins ? launch_analyse_as<L, true>(st, signal, window, twiddle, out, hop, frames, scale_half)                    \
                    : launch_analyse_as<L, false>(st, signal, window, twiddle, out, hop, frames, scale_half);
    switch (log2n) {
        SOTS_ANALYSE_CASE(8)
        SOTS_ANALYSE_CASE(9)
        SOTS_ANALYSE_CASE(10)
        SOTS_ANALYSE_CASE(11)
        SOTS_ANALYSE_CASE(12)
        SOTS_ANALYSE_CASE(13)
        SOTS_ANALYSE_CASE(14)
        SOTS_ANALYSE_CASE(15)
    default: return hipErrorInvalidValue;
    }
#undef SOTS_ANALYSE_CASE
}

hipError_t launch_score_frames(hipStream_t st, const float2 *bins, const float *targets, float *fitness, uint32_t log2n, uint32_t frames,
                               const Objective &obj)
{
    if (!bins || !targets || !fitness || frames == 0 || log2n < 8 || log2n > 15) return hipErrorInvalidValue;
    const uint32_t m = (1u << log2n) / 2u;
    const bool log = obj.kind == SOTS_OBJECTIVE_LOG_MAGNITUDE;
    if (obj.weights) {
        if (log) return launch_score_as<kObjLogMagnitude, true>(st, bins, targets, obj.weights, fitness, m, frames, obj.floor);
        return launch_score_as<kObjMagnitude, true>(st, bins, targets, obj.weights, fitness, m, frames, obj.floor);
    }
    if (log) return launch_score_as<kObjLogMagnitude, false>(st, bins, targets, nullptr, fitness, m, frames, obj.floor);
    return launch_score_as<kObjMagnitude, false>(st, bins, targets, nullptr, fitness, m, frames, obj.floor);
}

hipError_t analyse_reserve(AnalyseScratch &as, size_t signal_floats, size_t out_floats, size_t fitness_floats)
{
    if (hipError_t e = grow(as.signal, as.signal_floats, signal_floats)) return e;
    if (hipError_t e = grow(as.out, as.out_floats, out_floats)) return e;
    return grow(as.fitness, as.fitness_floats, fitness_floats);
}

void analyse_release(AnalyseScratch &as)
{
    for (float *b : {as.signal, as.out, as.fitness})
        if (b) (void)hipFree(b);
    as = AnalyseScratch{};
}

} // namespace sots
