// objective.h -- what turns a bin into its share of the fitness (bin_error, bin_error2), the helper that reads a kernel's
// trailing arguments, the derived table of the log objective and the segmented-target accessors.
#pragma once
#include "common.h"

// contraction: on for the magnitude forms (they are part of the arithmetic of the spectral kernels that call them), off
// for the log forms, bracketed below
#pragma clang fp contract(on)
namespace sots { namespace {

// ---- the selectable objective (sots_set_objective) ----
// OBJ is a template parameter of every kernel that turns bins into fitness.  kObjMagnitude is the reference's sum, and its
// instantiations are the kernels as they were: no extra argument, no extra instruction.  kObjLogMagnitude:
// sum_k (ln(m_k + floor) - ln(t_k + floor))^2 with m_k = |X_k| scale.  The kernels read a target table that already holds
// ln(t_k + floor), in whatever layout they read the magnitudes in (k_objective_map below made it with obj_ln_floor, the
// routine of the epilogues: a bin whose magnitude equals the target's contributes exactly 0, and nobody's log but
// v_log_f32's is involved).  The floor is one more kernel argument of the log instantiations only, behind all others.
constexpr int kObjMagnitude = SOTS_OBJECTIVE_MAGNITUDE, kObjLogMagnitude = SOTS_OBJECTIVE_LOG_MAGNITUDE;
// (host side: the table inside a weight image, launch_weight_image)
static inline const float *weight_table(const float *image) { return image + kSegTargetHeadFloats; }
#pragma clang fp contract(off) // (m + floor and log2 x ln 2 round one by one, here and in the table's kernel)
// ln(m + floor): v_log_f32 (log2, 1 ulp) times ln 2.  m >= 0 and 1e-30 <= floor <= 1 keep the argument a normal number,
// which is all that instruction handles; NaN and +inf pass through.
__device__ __forceinline__ float obj_ln_floor(float m, float floor)
{
    return __builtin_amdgcn_logf(m + floor) * 0.693147180559945f;
}
#pragma clang fp contract(on) // (back to the mode of the spectral kernels: the magnitude forms below are part of their arithmetic)

// ---- per-bin weights (sots_set_objective_weights) ----
// WGT is the second template parameter of those kernels: F = sum_k (u_k e_k)^2 with e_k the signed error of the objective
// and u_k = sqrt(w_k), a table made once on the host - one product, rounded once, and the squared accumulation as it stands.
// u = 1 gives the unweighted bits, u = 0 makes a finite bin contribute exactly 0.  The weighted instantiations take the table
// as one more trailing argument, behind the floor; the others are the kernels as they were.
//
// The pair below is the one statement of a bin's share: every fused and staged kernel calls it, so fused fitness equals
// staged fitness bit for bit.
// magnitude: (|X| * scale - target)^2 with scale = 1 / N / windowFactor, Evolutionary_Strategy.hpp:517-519 /
// ocl_program.cl:608-611 (one combined factor: 1/N is a power of two and the window factor is 1 to an ulp).
// v_sqrt_f32 (1 ulp) instead of the correctly rounded sequence: the transform feeding it is
// fp32 against the oracle's fp64 anyway.  The fused kernels pass 2 X and scale / 2: the same value bit for bit.
template <int OBJ, bool WGT>
__device__ __forceinline__ float bin_error(float2 x, float target, float scale, [[maybe_unused]] float floor, [[maybe_unused]] float u)
{
    const float raw = __builtin_amdgcn_sqrtf(x.x * x.x + x.y * x.y);
    if constexpr (OBJ == kObjLogMagnitude) {
#pragma clang fp contract(off) // (obj_ln_floor's mode: the target table was made by these operations, one rounding each;
                               // the pragma holds to the end of this block, the magnitude branch keeps the file's mode)
        float e = obj_ln_floor(raw * scale, floor) - target;
        if constexpr (WGT) e = e * u;
        return e * e;
    } else {
        float e = raw * scale - target;
        if constexpr (WGT) e = e * u;
        return e * e;
    }
}

// Two bins at once, each with its own running sum: the magnitudes come out of v_sqrt_f32 one by one, the scale, the
// subtraction and the squared accumulation are packed (acc2 = (sum over the bins k, sum over the bins M - k); k_fft<., 1> and
// k_fitness add the two halves in the same order, so both paths still give the same fp32 sum).  The log form packs floor
// and ln 2 as well; lane by lane the operations and their order are obj_ln_floor's.
template <int OBJ, bool WGT>
__device__ __forceinline__ void bin_error2(v2f_t &acc2, float2 xa, float2 xb, float ta, float tb, float scale, [[maybe_unused]] float floor,
                                           [[maybe_unused]] float ua, [[maybe_unused]] float ub)
{
    const v2f_t raw = v2f_t{__builtin_amdgcn_sqrtf(xa.x * xa.x + xa.y * xa.y), __builtin_amdgcn_sqrtf(xb.x * xb.x + xb.y * xb.y)};
    if constexpr (OBJ == kObjLogMagnitude) {
#pragma clang fp contract(off) // (as in bin_error; the pragma holds to the end of this block, not of the function)
        const v2f_t a = raw * v2f_t{scale, scale} + v2f_t{floor, floor};
        const v2f_t l = v2f_t{__builtin_amdgcn_logf(a.x), __builtin_amdgcn_logf(a.y)} * v2f_t{0.693147180559945f, 0.693147180559945f};
        v2f_t e = l - v2f_t{ta, tb};
        if constexpr (WGT) e = e * v2f_t{ua, ub};
        acc2 = acc2 + e * e;
    } else {
        v2f_t e = raw * v2f_t{scale, scale} - v2f_t{ta, tb};
        if constexpr (WGT) e = v2f_t{ua, ub} * e; // (u first: the operand order k_fitness was built with - the same bits, and the same bytes)
        acc2 = acc2 + e * e;
    }
}

// The argument of type T among a kernel's trailing arguments, or `none` where it has none.  The spectral kernels end in a
// pack that holds, in this order and each only in the instantiations that use it, the selection lists (SelLists, k_fft's
// BUCKET form), the floor (float, the log objective) and the weight table (const float *, the weighted forms): the other
// instantiations keep their argument list, and with it their code, to the byte.
template <typename T, typename D>
__device__ __forceinline__ D trailing(D none) { return none; }
template <typename T, typename D, typename A, typename... R>
__device__ __forceinline__ auto trailing(D none, A a, R... r)
{
    if constexpr (std::is_same_v<A, T>) return a;
    else return trailing<T>(none, r...);
}
// target[i] -> ln(target[i] + floor): the derived table of the log objective, plain bins (every other layout is copied from it)
__global__ __launch_bounds__(256) void k_objective_map(float *__restrict__ dst, const float *__restrict__ src, size_t n, float floor)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = obj_ln_floor(src[i], floor);
}

// Segmented target image (chunks in flight): word 0 holds the rows per chunk, the chunks' tables follow from float
// kSegHead on, `stride` floats each - the N/2 bins for k_fft and k_fft_big, k_fft_x's per-(lane, register) target
// table for k_fft_x (x_seg_stride).  Row r reads the table of chunk r / rows.
constexpr uint32_t kSegHead = kSegTargetHeadFloats; // (256 bytes: the tables start aligned)
__device__ __forceinline__ uint32_t seg_target_rows(const float *image)
{
    return __builtin_amdgcn_readfirstlane(reinterpret_cast<const uint32_t *>(image)[0]);
}
__device__ __forceinline__ const float *seg_target_chunk(const float *image, uint32_t chunk, uint32_t stride)
{
    return image + kSegHead + (size_t)chunk * stride;
}

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
