// window.h -- k_window: the analysis window over the audio rows (stage-separated path).
#pragma once
#include "common.h"

// contraction: off (the translation unit's default: one multiply per sample)
#pragma clang fp contract(off)
namespace sots { namespace {

// ------------------------------------------------------------------------------------
// applyWindowPopulation, ocl_program.cl:566-586.  The table is the reference's double
// window (Evolutionary_Strategy.hpp:308-317) rounded once to fp32.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_window(float *__restrict__ audio, const float *__restrict__ window,
                                                size_t total4, uint32_t log2n4, uint32_t pitch4)
{
    float4 *a4 = reinterpret_cast<float4 *>(audio);
    const float4 *w4 = reinterpret_cast<const float4 *>(window);
    const uint32_t mask = (1u << log2n4) - 1u;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total4;
         e += (size_t)gridDim.x * blockDim.x) {
        const size_t row = e >> log2n4;
        const uint32_t col = (uint32_t)e & mask;
        float4 v = a4[row * pitch4 + col];
        const float4 w = w4[col];
        v.x *= w.x; v.y *= w.y; v.z *= w.z; v.w *= w.w;
        a4[row * pitch4 + col] = v;
    }
}

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
