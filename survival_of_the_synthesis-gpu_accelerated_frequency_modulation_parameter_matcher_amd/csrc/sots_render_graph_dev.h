// sots_render_graph_dev.h -- what the two phase-continuous renderers of the operator-graph voice share on the device
// (sots_render_graph_continuous.hip; sots_render_graph_feedback.hip): the topology as kernel
// arguments, where a sample takes its genes, the scaling of a parameter, the shapes on the integer index and a lane's quad of
// an operator's phase words.  Moved here verbatim from sots_render_graph_continuous.hip.  Everything is in an anonymous
// namespace: each of the two files has its own copy, and nothing here is visible outside them.  Internal to libsots_hip.so.
#pragma once

#include "sots_render.h"

#pragma clang fp contract(off)

namespace sots {

namespace {

struct GraphTopo {
    uint32_t ops, carriers, shapes; // shapes: the codes, 3 bits per operator
    uint32_t modulators[8];
};

// Where sample n of the rendering takes its genes: row `a` (HOLD) or rows `a` and a + D at t between them (GLIDE)
struct GraphSample {
    const float *a;
    float t;
    bool lerp;
};
__device__ inline GraphSample gcont_sample(const GraphContPass &ps, uint32_t d, uint32_t n)
{
    uint32_t k, r;
    cont_position(n, ps.half_n, ps.hop, ps.num_rows, k, r);
    GraphSample s;
    s.lerp = ps.glide && r != 0u;
    if (!ps.glide) k += 2u * r >= ps.hop ? 1u : 0u;
    s.a = ps.values + (size_t)(k - ps.row_base) * d;
    s.t = s.lerp ? (float)r / (float)ps.hop : 0.0f;
    return s;
}
// parameter g of the sample, scaled as the graph voice scales it: no folding of the ranges
__device__ inline float gcont_param(const GraphContPass &ps, const GraphSample &s, uint32_t d, uint32_t g)
{
    float v = s.a[g];
    if (s.lerp) v = v + s.t * (s.a[g + d] - v);
    return ps.sp.pmin[g] + v * (ps.sp.pmax[g] - ps.sp.pmin[g]);
}

// shape(w, i) of four indices, every case decided on the integer index (include/sots_hip.h).  w is wavefront-uniform.
// Without the table (TABLE false) the host has seen to it that w is SQUARE or SAW.
template <bool TABLE> __device__ inline void gcont_shape(uint32_t w, const uint32_t at[4], const float *tab, float tv[4])
{
    constexpr uint32_t H = kWavetableSize / 2u, Q = kWavetableSize / 4u, M = kWavetableSize - 1u;
    if (w == SOTS_WAVE_SAW) {
#pragma unroll
        for (int e = 0; e < 4; ++e) tv[e] = (float)at[e] * 0x1p-14f - 1.0f;
        return;
    }
    if (!TABLE || w == SOTS_WAVE_SQUARE) {
#pragma unroll
        for (int e = 0; e < 4; ++e) tv[e] = at[e] < H ? 1.0f : -1.0f;
        return;
    }
    if constexpr (TABLE) {
        switch (w) {
        case SOTS_WAVE_HALF:
#pragma unroll
            for (int e = 0; e < 4; ++e) tv[e] = at[e] < H ? tab[at[e]] : 0.0f;
            break;
        case SOTS_WAVE_ABS:
#pragma unroll
            for (int e = 0; e < 4; ++e) tv[e] = fabsf(tab[at[e]]);
            break;
        case SOTS_WAVE_PULSE:
#pragma unroll
            for (int e = 0; e < 4; ++e) tv[e] = (at[e] & Q) == 0u ? fabsf(tab[at[e]]) : 0.0f;
            break;
        case SOTS_WAVE_EVEN: // (the read stays inside the table whatever the index; the upper half is +0)
#pragma unroll
            for (int e = 0; e < 4; ++e) tv[e] = at[e] < H ? tab[(2u * at[e]) & M] : 0.0f;
            break;
        case SOTS_WAVE_ABS_EVEN:
#pragma unroll
            for (int e = 0; e < 4; ++e) tv[e] = at[e] < H ? fabsf(tab[(2u * at[e]) & M]) : 0.0f;
            break;
        default:
#pragma unroll
            for (int e = 0; e < 4; ++e) tv[e] = tab[at[e]];
            break;
        }
    }
}

// this lane's quad of operator i's phase words, as table indices (0 behind the pass's end)
__device__ inline void gcont_indices(const GraphContPass &ps, uint32_t i, uint32_t first, uint32_t at[4])
{
    const uint32_t *buf = ps.words + (size_t)i * ps.lay.stride;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (first + 4u <= ps.count) {
        const uint4 q = *reinterpret_cast<const uint4 *>(buf + first);
        w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
    } else {
#pragma unroll
        for (uint32_t e = 0; e < 4u; ++e)
            if (first + e < ps.count) w[e] = buf[first + e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) at[e] = w[e] >> 17;
}

// The rows of this lane's quad.  A sample behind the pass's end takes the pass's last sample's: rows that are on the device.
__device__ inline void gcont_samples(const GraphContPass &ps, uint32_t d, uint32_t first, GraphSample sm[4])
{
#pragma unroll
    for (uint32_t e = 0; e < 4u; ++e) {
        const uint32_t at = first + e < ps.count ? first + e : ps.count - 1u;
        sm[e] = gcont_sample(ps, d, ps.n0 + at);
    }
}

} // namespace

} // namespace sots
