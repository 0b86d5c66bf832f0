// sots_track.h -- the run record a context (one chunk) and a batch (max_chunks chunks) keep on the device: best-ever
// individual, per-generation history ring, and the small read-back the stop rules look at.  Host side only; the kernel is
// k_track (kernels/track.h).  Internal to libsots_hip.so.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>

#include "../../include/sots_hip.h"
#include "sots_kernels.h"

namespace sots {

static_assert(sizeof(sots_gen_record) == kTrackRecordFloats * sizeof(float), "sots_gen_record is what k_track writes");

struct TrackState {
    uint32_t flags = 0;    // enum sots_track_flags; 0: nothing allocated, nothing launched
    uint32_t every = 0;    // history: a record when the generation counter is a multiple of this
    uint32_t capacity = 0; // history ring, records per chunk
    uint32_t chunks = 0;
    uint64_t taken = 0;    // records since the last clear (every chunk takes them together)
    uint32_t *meta = nullptr; // device uint32[chunks][2]
    float *rows = nullptr;    // device float[chunks][kTrackRowFloats]
    float *hist = nullptr;    // device float[chunks][capacity][kTrackRecordFloats]
    uint32_t *pinned = nullptr; // host uint32[chunks][2]: the stop rules' read-back

    bool best_ever() const { return (flags & SOTS_TRACK_BEST_EVER) != 0; }
    bool history() const { return (flags & SOTS_TRACK_HISTORY) != 0; }
};

inline void track_release(TrackState &t)
{
    if (t.meta) (void)hipFree(t.meta);
    if (t.rows) (void)hipFree(t.rows);
    if (t.hist) (void)hipFree(t.hist);
    if (t.pinned) (void)hipHostFree(t.pinned);
    t = TrackState{};
}

// the records of every chunk back to "nothing seen"; the history needs no device work (taken bounds what is read)
inline hipError_t track_clear(TrackState &t, hipStream_t st)
{
    t.taken = 0;
    if (!t.flags) return hipSuccess;
    return launch_track_clear(st, t.meta, t.rows, t.chunks);
}

// flags already normalised (HISTORY implies BEST_EVER) and checked; the caller has synchronised the stream
inline hipError_t track_setup(TrackState &t, uint32_t flags, uint32_t every, uint32_t capacity, uint32_t chunks, hipStream_t st)
{
    track_release(t);
    if (!flags) return hipSuccess;
    hipError_t e;
    if ((e = hipMalloc((void **)&t.meta, (size_t)chunks * 2 * sizeof(uint32_t))) != hipSuccess) return track_release(t), e;
    if ((e = hipMalloc((void **)&t.rows, (size_t)chunks * kTrackRowFloats * sizeof(float))) != hipSuccess) return track_release(t), e;
    if ((e = hipHostMalloc((void **)&t.pinned, (size_t)chunks * 2 * sizeof(uint32_t), hipHostMallocDefault)) != hipSuccess)
        return track_release(t), e;
    if (flags & SOTS_TRACK_HISTORY) {
        const size_t bytes = (size_t)chunks * capacity * sizeof(sots_gen_record);
        if ((e = hipMalloc((void **)&t.hist, bytes)) != hipSuccess) return track_release(t), e;
        if ((e = hipMemsetAsync(t.hist, 0, bytes, st)) != hipSuccess) return track_release(t), e;
    }
    t.flags = flags;
    t.every = (flags & SOTS_TRACK_HISTORY) ? every : 0;
    t.capacity = (flags & SOTS_TRACK_HISTORY) ? capacity : 0;
    t.chunks = chunks;
    if ((e = track_clear(t, st)) != hipSuccess) return track_release(t), e;
    return hipSuccess;
}

// after a generation's sort: `generation` is the counter after it, values / steps / fitness the half it wrote
inline hipError_t track_record(TrackState &t, hipStream_t st, const float *values, const float *steps, const float *fitness, uint32_t p,
                               uint32_t d, uint32_t parents, uint32_t generation, uint32_t active)
{
    if (!t.flags) return hipSuccess;
    uint32_t slot = kTrackNoSlot;
    if (t.history() && generation % t.every == 0) slot = (uint32_t)(t.taken % t.capacity);
    const hipError_t e = launch_track(st, values, steps, fitness, p, d, parents, generation, active, t.meta, t.rows, t.hist, t.capacity, slot);
    if (e == hipSuccess && slot != kTrackNoSlot) t.taken += 1;
    return e;
}

// {fitness bits, generation} of the first `active` chunks into t.pinned: a small asynchronous copy and a stream synchronise
inline hipError_t track_fetch_meta(TrackState &t, hipStream_t st, uint32_t active)
{
    hipError_t e = hipMemcpyAsync(t.pinned, t.meta, (size_t)active * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(st);
}

inline float track_fitness(const TrackState &t, uint32_t chunk)
{
    float f;
    memcpy(&f, &t.pinned[2 * chunk], sizeof f);
    return f;
}

// the newest min(taken, ring, out_capacity) records of one chunk, oldest first; blocking
inline hipError_t track_read_history(TrackState &t, hipStream_t st, uint32_t chunk, sots_gen_record *out, uint32_t out_capacity,
                                     uint32_t *written)
{
    const uint64_t held = t.taken < t.capacity ? t.taken : t.capacity;
    const uint32_t n = (uint32_t)(held < out_capacity ? held : out_capacity);
    *written = n;
    if (n == 0) return hipSuccess;
    const sots_gen_record *ring = reinterpret_cast<const sots_gen_record *>(t.hist) + (size_t)chunk * t.capacity;
    const uint32_t first = (uint32_t)((t.taken - n) % t.capacity); // the oldest of the n
    const uint32_t head = t.capacity - first < n ? t.capacity - first : n;
    hipError_t e = hipMemcpyAsync(out, ring + first, (size_t)head * sizeof(sots_gen_record), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) return e;
    if (head < n) {
        e = hipMemcpyAsync(out + head, ring, (size_t)(n - head) * sizeof(sots_gen_record), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return e;
    }
    return hipStreamSynchronize(st);
}

} // namespace sots
