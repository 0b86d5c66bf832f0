// sots_render.h -- overlap-add resynthesis of a parameter track (sots_render.hip).
// Internal to libsots_hip.so; the public boundary is sots_render_overlap_add in include/sots_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

namespace sots {

// One pass of the rendering.  The pass holds the audio of chunks first_row .. first_row + rows - 1 in `audio`, a row
// per chunk, `pitch` floats apart; positions are counted from the first sample of chunk first_row ("pass samples":
// chunk l of the pass stands for pass samples [l hop, l hop + n)).  The kernel writes out[j], j < 4 quads, for pass
// samples out_first + j: every chunk of the pass that covers the sample, in ascending order,
//     acc = acc + w[s - l hop] * a_l[s - l hop],  den = den + w[s - l hop],   out = den > 0 ? acc / den : 0
// with w = 1 where window == nullptr.  The caller sees to it that no chunk outside the pass covers a sample it keeps.
// out_first must be a multiple of 4 where hop is (the 16-byte row loads rest on it); out holds 4 quads floats.
struct RenderPass {
    const float *audio;
    const float *window; // N floats, or nullptr: rectangular
    float *out;
    uint32_t rows, hop, n, pitch;
    uint32_t out_first, quads;
};
hipError_t launch_overlap_add(hipStream_t st, const RenderPass &pass);

// Rows a pass may hold whatever the caller asks for: the pass samples stay far below 2^31 and the scratch below 256 MiB.
inline uint32_t render_max_rows(uint32_t pitch)
{
    const uint32_t r = (1u << 26) / pitch;
    return r < 128u ? 128u : r;
}

// Device memory of the rendering, owned by a context: allocated on first use, grown when a call needs more, freed
// with the context.  Apart from these three buffers a rendering writes nothing on the device.
struct RenderScratch {
    float *values = nullptr, *audio = nullptr, *out = nullptr;
    size_t values_floats = 0, audio_floats = 0, out_floats = 0;
};
hipError_t render_reserve(RenderScratch &rs, size_t values_floats, size_t audio_floats, size_t out_floats);
void render_release(RenderScratch &rs);

} // namespace sots
