// Driver for the sanitizer build of the host-only code behind carried rows in the chunk queue (sots_batch_queue_set_carry):
// queue_carry_check and its refusal texts, the layout of a run (queue_plan), the turnover's segment arithmetic
// (queue_has_successor, queue_segment_start: the copy the kernel compiles) played through by a host model of the slots,
// and the loop bound.  Built and run by tests/test_queue_carry_cpu.py under ASan + UBSan; host code only.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/sots_hip.h"
#include "../survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd/csrc/sots_rules.h"
#include "../survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd/csrc/sots_stop_rule.h"

using namespace sots;

static const uint32_t kNone = 0xFFFFFFFFu;

// the definition, in the header's words: segment g holds chunks [g L, (g + 1) L), and chunk k with k % L != 0 is a successor
static uint32_t queue_segment_of(const QueuePlan &p, uint32_t chunk) { return chunk / p.segment; }
static bool queue_is_successor(const QueuePlan &p, uint32_t chunk) { return chunk % p.segment != 0u; }

// The queue loop as the turnover kernel plays it: every loop generation each busy slot advances its chunk by one; a slot
// whose chunk has run its generations retires it and takes the successor, or draws a segment from the head.  Slots that
// retire in the same generation draw in slot order (any order gives the same makespan: they are interchangeable).
// Returns the loop generation of the last retirement; slot_of / started_at say where and when each chunk started.
static uint64_t play(const QueuePlan &p, uint32_t carry_rows, const std::vector<uint32_t> &run, std::vector<uint32_t> &slot_of,
                     std::vector<uint64_t> &started_at, int &bad)
{
    const uint32_t chunks = (uint32_t)run.size();
    const uint32_t segment = carry_rows ? p.segment : 1u, segments = carry_rows ? p.segments : chunks;
    std::vector<uint32_t> chunk_of(p.slots), done(p.slots, 0);
    slot_of.assign(chunks, kNone);
    started_at.assign(chunks, 0);
    uint32_t head = p.slots, retired = 0;
    for (uint32_t c = 0; c < p.slots; ++c) {
        chunk_of[c] = c * p.segment;
        slot_of[chunk_of[c]] = c;
    }
    uint64_t global = 0, last = 0;
    while (retired < chunks) {
        global += 1;
        if (global > (1ull << 40)) return bad += 1, 0;
        for (uint32_t c = 0; c < p.slots; ++c) {
            const uint32_t chunk = chunk_of[c];
            if (chunk == kNone) continue;
            if (++done[c] < run[chunk]) continue;
            retired += 1;
            last = global;
            uint32_t next;
            if (queue_has_successor(chunk, segment, chunks)) next = chunk + 1u;
            else next = queue_segment_start(head++, segment, segments, kNone);
            chunk_of[c] = next < chunks ? next : kNone;
            done[c] = 0;
            if (next < chunks) {
                bad += slot_of[next] != kNone; // started twice
                slot_of[next] = c;
                started_at[next] = global;
            }
        }
    }
    return last;
}

int main()
{
    int bad = 0;
    // ---- queue_carry_check ----
    bad += (bool)queue_carry_check(0, 0, 16) || (bool)queue_carry_check(0, 7, 16) || (bool)queue_carry_check(0, 0, 0);
    bad += (bool)queue_carry_check(1, 1, 16) || (bool)queue_carry_check(16, 0xFFFFFFFFu, 16);
    Fault f = queue_carry_check(17, 4, 16);
    bad += f.code != SOTS_ERR_INVALID || !strstr(f.text, "17") || !strstr(f.text, "numParents = 16");
    f = queue_carry_check(0xFFFFFFFFu, 4, 16);
    bad += f.code != SOTS_ERR_INVALID || !strstr(f.text, "4294967295");
    f = queue_carry_check(3, 0, 16);
    bad += f.code != SOTS_ERR_INVALID || !strstr(f.text, "segment_chunks");
    f = queue_carry_check(1, 1, 0);
    bad += f.code != SOTS_ERR_INVALID;

    // ---- queue_plan: hand cases ----
    QueuePlan p = queue_plan(13, 4, 0, 0); // carry off: a chunk is a segment
    bad += p.segment != 1 || p.segments != 13 || p.slots != 4;
    p = queue_plan(13, 4, 0, 5); // ... whatever the length says
    bad += p.segment != 1 || p.segments != 13 || p.slots != 4;
    p = queue_plan(13, 4, 1, 3);
    bad += p.segment != 3 || p.segments != 5 || p.slots != 4;
    p = queue_plan(13, 8, 2, 3);
    bad += p.segment != 3 || p.segments != 5 || p.slots != 5;
    p = queue_plan(13, 4, 1, 13);
    bad += p.segment != 13 || p.segments != 1 || p.slots != 1;
    p = queue_plan(13, 4, 1, 20); // longer than the queue: one segment of all its chunks
    bad += p.segment != 13 || p.segments != 1 || p.slots != 1;
    p = queue_plan(13, 4, 1, 0xFFFFFFFFu);
    bad += p.segment != 13 || p.segments != 1 || p.slots != 1;
    p = queue_plan(13, 4, 16, 1); // no successors
    bad += p.segment != 1 || p.segments != 13 || p.slots != 4;
    p = queue_plan(0xFFFFFFFFu, 0xFFFFFFFFu, 1, 0xFFFFFFFEu);
    bad += p.segment != 0xFFFFFFFEu || p.segments != 2 || p.slots != 2;
    p = queue_plan(1, 16, 1, 1);
    bad += p.segment != 1 || p.segments != 1 || p.slots != 1;
    p = queue_plan(13, 4, 1, 3);
    bad += queue_is_successor(p, 0) || !queue_is_successor(p, 1) || !queue_is_successor(p, 2) || queue_is_successor(p, 3) || queue_is_successor(p, 12);
    bad += queue_segment_of(p, 2) != 0 || queue_segment_of(p, 3) != 1 || queue_segment_of(p, 12) != 4;

    // ---- the turnover's arithmetic at the edges ----
    bad += queue_has_successor(2, 3, 13) || !queue_has_successor(3, 3, 13) || queue_has_successor(12, 3, 13) || queue_has_successor(12, 20, 13);
    bad += queue_has_successor(0, 1, 13) || queue_has_successor(0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu) || !queue_has_successor(0xFFFFFFFDu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    bad += queue_segment_start(4, 3, 5, kNone) != 12 || queue_segment_start(5, 3, 5, kNone) != kNone || queue_segment_start(kNone, 3, 5, kNone) != kNone;
    bad += queue_segment_start(1, 0xFFFFFFFEu, 2, kNone) != 0xFFFFFFFEu;

    // ---- the loop bound: hand cases, then saturation ----
    p = queue_plan(13, 4, 0, 0);
    bad += queue_loop_bound(p, 200, true) != (12 / 4 + 2) * 200ull || queue_loop_bound(p, 200, false) != 4 * 200ull; // as without carrying
    p = queue_plan(13, 4, 1, 3);
    bad += queue_loop_bound(p, 200, true) != ((5 - 1) / 4 + 2) * 3 * 200ull || queue_loop_bound(p, 200, false) != 2 * 3 * 200ull;
    p = queue_plan(13, 4, 1, 20);
    bad += queue_loop_bound(p, 200, true) != 2 * 13 * 200ull || queue_loop_bound(p, 200, false) != 13 * 200ull;
    p = queue_plan(0xFFFFFFFFu, 1, 1, 0xFFFFu);
    bad += queue_loop_bound(p, 0xFFFFFFFFu, true) != ~0ull; // 65538 rounds of 0xFFFF * 0xFFFFFFFF generations: beyond 64 bits
    p = queue_plan(0xFFFFFFFFu, 1, 0, 0);
    bad += queue_loop_bound(p, 0xFFFFFFFFu, false) != 0xFFFFFFFFull * 0xFFFFFFFFull;

    // ---- seeded random runs: every chunk starts once, a successor where and when its predecessor ended, the makespan is
    // that of the segments' sums, and the loop bound holds it ----
    uint64_t x = 0x5EED0001ull;
    auto next = [&x]() { return (uint32_t)((x = x * 6364136223846793005ull + 1442695040888963407ull) >> 33); };
    int cases = 0;
    for (; cases < 300; ++cases) {
        const uint32_t m = 1 + next() % 60, max_chunks = 1 + next() % 12, rows = next() % 3, len = 1 + next() % 24;
        const uint32_t interval = 1 + next() % 5, max_g = interval * (1 + next() % 6) + (next() % 2 ? next() % interval : 0);
        const bool with_rule = next() % 3 != 0;
        std::vector<uint32_t> run(m);
        for (uint32_t &r : run) {
            r = with_rule ? interval * (1 + next() % 8) : max_g; // a rule stops at a boundary, or max_generations does
            if (r > max_g) r = max_g;
        }
        const QueuePlan plan = queue_plan(m, max_chunks, rows, len);
        bad += plan.segment == 0 || plan.slots == 0 || plan.slots > max_chunks || plan.slots > plan.segments;
        bad += (uint64_t)(plan.segments - 1) * plan.segment >= m || (uint64_t)plan.segments * plan.segment < m;
        if (rows == 0) bad += plan.segment != 1 || plan.segments != m;
        std::vector<uint32_t> slot_of;
        std::vector<uint64_t> started_at;
        const uint64_t span = play(plan, rows, run, slot_of, started_at, bad);
        std::vector<uint64_t> end_at(m);
        for (uint32_t k = 0; k < m; ++k) {
            bad += slot_of[k] == kNone;
            end_at[k] = started_at[k] + run[k];
            if (queue_is_successor(plan, k)) bad += slot_of[k] != slot_of[k - 1] || started_at[k] != end_at[k - 1];
        }
        std::vector<uint32_t> sums(plan.segments, 0);
        for (uint32_t k = 0; k < m; ++k) sums[queue_segment_of(plan, k)] += run[k];
        uint64_t model = 0;
        bad += sots_queue_makespan(sums.data(), plan.segments, plan.slots, &model) != SOTS_OK || model != span;
        const uint64_t bound = queue_loop_bound(plan, max_g, with_rule);
        bad += span > bound;
        if (!with_rule && m % plan.segment == 0 && plan.segments % plan.slots == 0) bad += span != bound; // whole rounds: exactly the bound
    }
    printf("queue carry host code: %d random cases, %d failures\n", cases, bad);
    return bad ? 1 : 0;
}
