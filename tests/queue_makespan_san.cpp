// Driver for the sanitizer build of the chunk queue's host-only code (csrc/sots_queue_host.cpp, csrc/sots_stop_rule.h):
// sots_queue_makespan on hand cases and on seeded random ones against a plain O(M S) model, and the shared stop-rule
// arithmetic.  Built and run by tests/test_chunk_queue_cpu.py under ASan + UBSan; host code only.
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../include/sots_hip.h"
#include "../survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd/csrc/sots_stop_rule.h"

static uint64_t model(const std::vector<uint32_t> &g, uint32_t slots)
{
    std::vector<uint64_t> free_at(slots, 0);
    uint64_t last = 0;
    for (uint32_t r : g) {
        size_t best = 0;
        for (size_t s = 1; s < free_at.size(); ++s)
            if (free_at[s] < free_at[best]) best = s;
        free_at[best] += r;
        if (free_at[best] > last) last = free_at[best];
    }
    return last;
}

int main()
{
    uint64_t out = 7;
    int bad = 0;
    const std::vector<uint32_t> hand = {75, 100, 125, 175, 75, 75};
    bad += sots_queue_makespan(hand.data(), 6, 1, &out) != SOTS_OK || out != 625;   // one slot: the sum
    bad += sots_queue_makespan(hand.data(), 6, 6, &out) != SOTS_OK || out != 175;   // slots >= chunks: the max
    bad += sots_queue_makespan(hand.data(), 6, 64, &out) != SOTS_OK || out != 175;
    bad += sots_queue_makespan(hand.data(), 6, 2, &out) != SOTS_OK || out != model(hand, 2);
    bad += sots_queue_makespan(nullptr, 0, 3, &out) != SOTS_OK || out != 0;         // no chunks
    bad += sots_queue_makespan(hand.data(), 6, 0, &out) != SOTS_ERR_INVALID;
    bad += sots_queue_makespan(nullptr, 6, 2, &out) != SOTS_ERR_INVALID;
    bad += sots_queue_makespan(hand.data(), 6, 2, nullptr) != SOTS_ERR_INVALID;
    const std::vector<uint32_t> huge(5, 0xFFFFFFFFu); // the sum leaves 32 bits
    bad += sots_queue_makespan(huge.data(), 5, 1, &out) != SOTS_OK || out != 5ull * 0xFFFFFFFFull;

    uint64_t x = 0x5EED0001ull;
    auto next = [&x]() { return (uint32_t)((x = x * 6364136223846793005ull + 1442695040888963407ull) >> 33); };
    int cases = 0;
    for (; cases < 300; ++cases) {
        const uint32_t m = next() % 200, s = 1 + next() % 40;
        std::vector<uint32_t> g(m);
        for (uint32_t &v : g) v = (next() % 4 == 0) ? 0 : 25 * (1 + next() % 40);
        bad += sots_queue_makespan(g.data(), m, s, &out) != SOTS_OK || out != model(g, s);
    }
    // the rule's arithmetic: saturating difference, NaN never reaches a target, both conditions off never hold
    bad += !sots::stop_rule_holds(-1.0f, 8, 1.0f, 2, 10) || sots::stop_rule_holds(-1.0f, 8, 1.0f, 3, 10);
    bad += sots::stop_rule_holds(-1.0f, 8, 1.0f, 0xFFFFFFFFu, 0);
    bad += sots::stop_rule_holds(0.5f, 0, std::numeric_limits<float>::quiet_NaN(), 0, 100) || !sots::stop_rule_holds(0.5f, 0, 0.5f, 0, 0);
    bad += sots::stop_rule_holds(-1.0f, 0, 0.0f, 0, 0xFFFFFFFFu);
    printf("queue host code: %d random cases, %d failures\n", cases, bad);
    return bad ? 1 : 0;
}
