// sots_stop_rule.h -- the arithmetic of the stop rules (sots_stop_rule, include/sots_hip.h) in ONE copy for the host
// (sots_stop_rule_holds, the block loops of sots_execute_until) and for the device (the chunk queue's turnover,
// k_queue_turnover), the turnover's segment arithmetic likewise, and the queue's makespan model.  No HIP header: plain C++ compilers build it too (the sanitizer
// builds of tests/).  Internal to libsots_hip.so.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <functional>
#include <queue>
#include <vector>

#if defined(__HIPCC__)
#define SOTS_HOST_DEVICE __host__ __device__
#else
#define SOTS_HOST_DEVICE
#endif

namespace sots {

// does the rule hold?  target_fitness < 0: no fitness target; stall_generations 0: no stall rule; both off: never.
// The difference of the generations saturates at 0; NaN is never <= a target.
SOTS_HOST_DEVICE inline bool stop_rule_holds(float target_fitness, uint32_t stall_generations, float best_ever_fitness,
                                             uint32_t best_ever_generation, uint32_t generation)
{
    if (target_fitness >= 0.0f && best_ever_fitness <= target_fitness) return true;
    if (stall_generations != 0) {
        const uint32_t since = generation > best_ever_generation ? generation - best_ever_generation : 0u;
        if (since >= stall_generations) return true;
    }
    return false;
}

// Carried rows (sots_batch_queue_set_carry): the queue's chunks in segments of `segment` (>= 1) consecutive chunks, the
// turnover's arithmetic.  Does the slot that retires `chunk` (< num_chunks) go on with chunk + 1, the next of its segment?
SOTS_HOST_DEVICE inline bool queue_has_successor(uint32_t chunk, uint32_t segment, uint32_t num_chunks)
{
    return (chunk + 1u) % segment != 0u && chunk + 1u < num_chunks; // (chunk + 1 <= num_chunks: no wrap)
}
// the first chunk of the segment a free slot drew from the head, or `none` where the head has passed the last segment
// (num_segments = ceil(num_chunks / segment), so seg * segment <= num_chunks - 1: no wrap)
SOTS_HOST_DEVICE inline uint32_t queue_segment_start(uint32_t seg, uint32_t segment, uint32_t num_segments, uint32_t none)
{
    return seg < num_segments ? seg * segment : none;
}

// The global generations an in-order refill of `slots` slots takes: every slot is free at generation 0, chunk k starts
// in the slot that is free first, at the generation at which it was freed.  Slots freed at the same generation are
// interchangeable, so which of them takes which chunk does not change the answer.
inline uint64_t queue_makespan(const uint32_t *generations_run, uint32_t num_chunks, uint32_t slots)
{
    std::priority_queue<uint64_t, std::vector<uint64_t>, std::greater<uint64_t>> free_at;
    for (uint32_t s = 0; s < slots && s < num_chunks; ++s) free_at.push(0);
    uint64_t last = 0;
    for (uint32_t k = 0; k < num_chunks; ++k) {
        const uint64_t end = free_at.top() + generations_run[k];
        free_at.pop();
        free_at.push(end);
        last = std::max(last, end);
    }
    return last;
}

} // namespace sots
