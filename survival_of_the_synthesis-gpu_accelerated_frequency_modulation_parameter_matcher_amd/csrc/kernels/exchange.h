// exchange.h -- the island exchange as launches of its own: k_pack_rows, k_unpack_rows (the kernels that move sorted rows
// carry it themselves: ex_*, sort.h).
#pragma once
#include "common.h"

// contraction: off (the translation unit's default: rows are copied, every float as it is)
#pragma clang fp contract(off)
namespace sots { namespace {

// ------------------------------------------------------------------------------------
// island exchange: rows of [fitness, values, steps]
// ------------------------------------------------------------------------------------
__global__ void k_pack_rows(const float *__restrict__ values, const float *__restrict__ steps,
                            const float *__restrict__ fitness, float *__restrict__ rows,
                            uint32_t first_row, uint32_t n_rows, uint32_t d)
{
    const uint32_t w = 2 * d + 1, total = n_rows * w;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t r = e / w, c = e - r * w, src = first_row + r;
        rows[e] = c == 0 ? fitness[src] : c <= d ? values[src * d + (c - 1)] : steps[src * d + (c - 1 - d)];
    }
}

// rows [skip_first, skip_first + skip_count) of the source are passed over (an island's own
// block inside an all-gathered buffer)
__global__ void k_unpack_rows(float *__restrict__ values, float *__restrict__ steps,
                              float *__restrict__ fitness, const float *__restrict__ rows,
                              uint32_t first_row, uint32_t n_rows, uint32_t d, uint32_t skip_first,
                              uint32_t skip_count)
{
    const uint32_t w = 2 * d + 1, total = n_rows * w;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t r = e / w, c = e - r * w, dst = first_row + r;
        const uint32_t sr = r < skip_first ? r : r + skip_count;
        const float v = rows[sr * w + c];
        if (c == 0) fitness[dst] = v;
        else if (c <= d) values[dst * d + (c - 1)] = v;
        else steps[dst * d + (c - 1 - d)] = v;
    }
}

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
