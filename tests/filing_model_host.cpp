// The two-level bucket lookup of the key-filing kernels (kernels/sel_keys.h, kBktTwoLevel) on the host, step by step as
// a wavefront takes it, through the index map and the count -> bucket formula of csrc/sots_bkt_layout.h - the one
// statement the kernels use.  tests/test_cpu_filing_model.py compares its answers with brute force.
//   stdin:  B, then B non-decreasing bounds (t_0 first), then n and n keys; all numbers in hex
//   stdout: the table index of bound q for q = 0 .. 255 on one line, then one bucket per key
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd/csrc/sots_bkt_layout.h"

int main()
{
    using namespace sots;
    constexpr uint32_t kBounds = kBktGroups * kBktGroupSize;
    uint32_t B = 0;
    if (scanf("%" SCNx32, &B) != 1 || B < 2 || B > kBounds) return 2;
    std::vector<uint64_t> table(kBounds, ~0ull); // bounds from B on: all-ones
    for (uint32_t q = 0; q < B; ++q) {
        uint64_t t;
        if (scanf("%" SCNx64, &t) != 1) return 2;
        table[bkt_slot_of(q)] = q == 0 ? 0ull : t;
    }
    for (uint32_t q = 0; q < kBounds; ++q) printf("%u%c", bkt_slot_of(q), q + 1 < kBounds ? ' ' : '\n');
    const uint64_t last = table[bkt_slot_of(B - 1)];
    uint32_t n = 0;
    if (scanf("%" SCNx32, &n) != 1) return 2;
    for (uint32_t i = 0; i < n; ++i) {
        uint64_t key;
        if (scanf("%" SCNx64, &key) != 1) return 2;
        if (key >= last) { // the open bucket
            printf("%u\n", B - 1);
            continue;
        }
        uint32_t groups = 0, inside = 0;
        for (uint32_t lane = 0; lane < kBktGroups; ++lane) groups += table[bkt_group_last(lane)] <= key;
        if (groups >= kBktGroups) return 3; // (the table's last bound is >= last > key)
        for (uint32_t lane = 0; lane < kBktGroupSize; ++lane) inside += table[bkt_slot_of(lane) + groups] <= key;
        printf("%u\n", bkt_bucket_of(groups, inside));
    }
    return 0;
}
