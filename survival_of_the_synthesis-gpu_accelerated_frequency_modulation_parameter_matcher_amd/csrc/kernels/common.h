// common.h -- what every kernel family uses: the wavefront size, packed-float and compile-time-index types and the
// cross-lane primitives (wavefront sum, value of lane ^ J); the synthesis kernels' wavetable on its way into LDS.
#pragma once
#include "../sots_kernels.h"
#include <type_traits>

// contraction: off (the translation unit's default; nothing here multiplies and adds)
#pragma clang fp contract(off)
namespace sots { namespace {

constexpr int kWave = 64;
typedef float v2f_t __attribute__((ext_vector_type(2)));

template <int V> using ic = std::integral_constant<int, V>;
// f(ic<I>{}) for I = FIRST .. LAST-1 with I a compile-time constant inside f (register arrays are indexed with it)
template <int FIRST, int LAST, typename F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (FIRST < LAST) {
        f(ic<FIRST>{});
        static_for<FIRST + 1, LAST>(f);
    }
}

// Wavefront sum without LDS traffic: DPP swaps inside each row of 16 lanes (every lane of a
// row ends with the row total), then the four row totals are added in row order.
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v)
{
    const int m = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false);
    return v + __int_as_float(m);
}
__device__ __forceinline__ float wave_sum(float v)
{
    v = dpp_add<0xB1>(v);  // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);  // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v); // row_half_mirror
    v = dpp_add<0x140>(v); // row_mirror
    const int iv = __float_as_int(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(iv, 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(iv, 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(iv, 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(iv, 48));
    return ((r0 + r1) + r2) + r3;
}

// value of lane (lane ^ J) for J = 1, 2 (DPP quad permutes), 4, 8, 16 (ds_swizzle through the LDS crossbar,
// no LDS memory), 32 (v_permlane32_swap)
template <uint32_t J>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v)
{
    if constexpr (J == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true); // quad_perm [1,0,3,2]
    else if constexpr (J == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, true); // quad_perm [2,3,0,1]
    else if constexpr (J == 32) {
        const auto sw = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return (threadIdx.x & 32u) ? sw[0] : sw[1]; // lanes 32-63 get lane-32's value in [0], lanes 0-31 lane+32's in [1]
    } else return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (int)((J << 10) | 0x1Fu)); // bit mode: xor J, and 0x1f
}
template <uint32_t J> __device__ __forceinline__ float lane_xor_f(float v)
{
    if constexpr (J == 8) return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x128, 0xf, 0xf, true)); // row_ror:8
    else return __uint_as_float(lane_xor<J>(__float_as_uint(v)));
}

// The synthesis kernels' wavetable, global -> LDS (every thread of the workgroup calls it; tab holds kWavetableSize floats)
__device__ __forceinline__ void request_wavetable(float *__restrict__ tab, const float *__restrict__ wavetable)
{
    // global -> LDS directly (global_load_lds_dwordx4): one wavefront instruction lands 1 KiB at a
    // wavefront-uniform LDS base + lane * 16 B, no registers in between, all 128 in flight at once
    typedef __attribute__((address_space(3))) void *lds_ptr_t;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x & (kWave - 1);
    const uint32_t waves = blockDim.x / kWave;
    constexpr uint32_t kChunk = kWave * 4; // floats per instruction
    for (uint32_t ch = wave; ch < kWavetableSize / kChunk; ch += waves)
        __builtin_amdgcn_global_load_lds(wavetable + ch * kChunk + lane * 4u, (lds_ptr_t)(tab + ch * kChunk), 16, 0, 0);
}
// ... and the wait for it, after whatever else the kernel can start meanwhile
__device__ __forceinline__ void wavetable_ready()
{
    __builtin_amdgcn_s_waitcnt(0); // vmcnt(0): the copies have landed
    __syncthreads();
}

// Audio rows are read exactly once per generation: non-temporal loads keep them from
// displacing other data in L2 / Infinity Cache (P = 131072: 151 -> 132 us; neutral at 65536).
typedef float v4f_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_load4(const float4 *p)
{
    const v4f_t v = __builtin_nontemporal_load(reinterpret_cast<const v4f_t *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
#define SOTS_ROW_LOAD(p) nt_load4(p)

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
