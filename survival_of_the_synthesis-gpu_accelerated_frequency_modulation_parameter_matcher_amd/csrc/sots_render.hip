// sots_render.hip -- overlap-add resynthesis (sots_render_overlap_add): the gather kernel that adds the
// windowed audio of the chunks covering each output sample, and the scratch it works from.
//
// A GATHER: a lane owns four consecutive output samples, walks the chunks that cover them in ascending order - at most
// 64, the hop is at least N / 64 - and stores its 16 bytes once.  The scatter form (a lane per synthesised sample adding
// into the output) needs float atomics, whose sums depend on arrival order; here the order of every sum is fixed by the
// loop, so the same inputs give the same bits on every run, with any pass size.  Every term is one fp32 multiply and one
// fp32 add, uncontracted, and the quotient is the correctly rounded fp32 division: what tests/_render_model.py states in
// NumPy.
#include "sots_render.h"

#pragma clang fp contract(off)

namespace sots {

namespace {

constexpr int kRenderThreads = 256;

// VEC: hop % 4 == 0.  The chunk bounds l hop and l hop + n are then multiples of 4 like the quad's first sample, so the
// four samples share their covering chunks and each chunk is one 16-byte row load (rows are pitch = n + 32 floats apart:
// 16-byte aligned).  Otherwise every sample has its own range of chunks and loads scalars.
template <bool VEC, bool WINDOWED>
__global__ __launch_bounds__(kRenderThreads) void k_overlap_add(RenderPass ps)
{
    const uint32_t stride = gridDim.x * kRenderThreads;
    for (uint32_t q = blockIdx.x * kRenderThreads + threadIdx.x; q < ps.quads; q += stride) {
        const uint32_t s = ps.out_first + 4u * q; // pass sample of the quad's first output
        float4 res;
        if constexpr (VEC) {
            // chunks l with l hop <= s < l hop + n, clipped to the pass
            const uint32_t lo = s >= ps.n ? (s - ps.n) / ps.hop + 1u : 0u;
            uint32_t hi = s / ps.hop;
            hi = hi < ps.rows - 1u ? hi : ps.rows - 1u;
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f), den = acc;
            for (uint32_t l = lo; l <= hi; ++l) { // (lo > hi: nobody covers the quad)
                const uint32_t off = s - l * ps.hop; // < n, a multiple of 4
                const float4 a = *reinterpret_cast<const float4 *>(ps.audio + (size_t)l * ps.pitch + off);
                if constexpr (WINDOWED) {
                    const float4 w = *reinterpret_cast<const float4 *>(ps.window + off);
                    acc.x = acc.x + w.x * a.x, acc.y = acc.y + w.y * a.y, acc.z = acc.z + w.z * a.z, acc.w = acc.w + w.w * a.w;
                    den.x = den.x + w.x, den.y = den.y + w.y, den.z = den.z + w.z, den.w = den.w + w.w;
                } else {
                    acc.x = acc.x + 1.0f * a.x, acc.y = acc.y + 1.0f * a.y, acc.z = acc.z + 1.0f * a.z, acc.w = acc.w + 1.0f * a.w;
                    den.x = den.x + 1.0f, den.y = den.y + 1.0f, den.z = den.z + 1.0f, den.w = den.w + 1.0f;
                }
            }
            res.x = den.x > 0.0f ? acc.x / den.x : 0.0f;
            res.y = den.y > 0.0f ? acc.y / den.y : 0.0f;
            res.z = den.z > 0.0f ? acc.z / den.z : 0.0f;
            res.w = den.w > 0.0f ? acc.w / den.w : 0.0f;
        } else {
            float r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t sk = s + (uint32_t)k;
                const uint32_t lo = sk >= ps.n ? (sk - ps.n) / ps.hop + 1u : 0u;
                uint32_t hi = sk / ps.hop;
                hi = hi < ps.rows - 1u ? hi : ps.rows - 1u;
                float acc = 0.0f, den = 0.0f;
                for (uint32_t l = lo; l <= hi; ++l) {
                    const uint32_t off = sk - l * ps.hop; // < n
                    const float a = ps.audio[(size_t)l * ps.pitch + off];
                    const float w = WINDOWED ? ps.window[off] : 1.0f;
                    acc = acc + w * a;
                    den = den + w;
                }
                r[k] = den > 0.0f ? acc / den : 0.0f;
            }
            res = make_float4(r[0], r[1], r[2], r[3]);
        }
        *reinterpret_cast<float4 *>(ps.out + 4u * (size_t)q) = res;
    }
}

} // namespace

hipError_t launch_overlap_add(hipStream_t st, const RenderPass &ps)
{
    if (!ps.audio || !ps.out || ps.rows == 0 || ps.hop == 0 || ps.hop > ps.n || (ps.n & 3u) || (ps.pitch & 3u) || ps.pitch < ps.n)
        return hipErrorInvalidValue;
    const bool vec = (ps.hop & 3u) == 0u;
    if (vec && (ps.out_first & 3u)) return hipErrorInvalidValue;
    // the last pass sample any lane looks at stays a 32-bit number
    if ((uint64_t)ps.out_first + 4ull * ps.quads + ps.n >= (1ull << 31) || (uint64_t)ps.rows * ps.hop >= (1ull << 31)) return hipErrorInvalidValue;
    if (ps.quads == 0) return hipSuccess;
    uint32_t grid = (ps.quads + kRenderThreads - 1) / kRenderThreads;
    grid = grid > 2048u ? 2048u : grid; // memory bound: the rest by grid stride
    if (vec) {
        if (ps.window) k_overlap_add<true, true><<<grid, kRenderThreads, 0, st>>>(ps);
        else k_overlap_add<true, false><<<grid, kRenderThreads, 0, st>>>(ps);
    } else {
        if (ps.window) k_overlap_add<false, true><<<grid, kRenderThreads, 0, st>>>(ps);
        else k_overlap_add<false, false><<<grid, kRenderThreads, 0, st>>>(ps);
    }
    return hipGetLastError();
}

hipError_t render_reserve(RenderScratch &rs, size_t values_floats, size_t audio_floats, size_t out_floats)
{
    auto grow = [](float *&buf, size_t &have, size_t need) -> hipError_t {
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
    };
    if (hipError_t e = grow(rs.values, rs.values_floats, values_floats)) return e;
    if (hipError_t e = grow(rs.audio, rs.audio_floats, audio_floats)) return e;
    return grow(rs.out, rs.out_floats, out_floats);
}

hipError_t render_reserve_words(RenderScratch &rs, size_t words)
{
    if (words <= rs.words_count) return hipSuccess;
    if (rs.words) {
        const hipError_t e = hipFree(rs.words);
        rs.words = nullptr, rs.words_count = 0;
        if (e != hipSuccess) return e;
    }
    const hipError_t e = hipMalloc((void **)&rs.words, words * sizeof(uint32_t));
    if (e != hipSuccess) return rs.words = nullptr, e;
    rs.words_count = words;
    return hipSuccess;
}

void render_release(RenderScratch &rs)
{
    for (float *b : {rs.values, rs.audio, rs.out})
        if (b) (void)hipFree(b);
    if (rs.words) (void)hipFree(rs.words);
    rs = RenderScratch{};
}

} // namespace sots
