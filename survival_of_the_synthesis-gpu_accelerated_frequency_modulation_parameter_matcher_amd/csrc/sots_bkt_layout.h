// sots_bkt_layout.h -- where the two-level key filing (kernels/sel_keys.h, kBktTwoLevel) keeps bound q of a slot, and the
// bucket that its two counts name: stated ONCE, for the kernels and for the host model of tests/.  No HIP header: plain
// C++ compilers build it too.  Internal to libsots_hip.so.
#pragma once

#include <stdint.h>

namespace sots {

// The bounds t_0 = 0 <= t_1 <= ... <= t_{B-1} <= all-ones ... (kBktGroups * kBktGroupSize of them, non-decreasing from end
// to end) lie in groups of four consecutive bounds, member c of every group side by side: lane l of a wavefront reads the
// c-th bound of group l, and lanes 0 .. 3 read the four bounds of one group, in one contiguous access each.
constexpr uint32_t kBktGroupSize = 4, kBktGroups = 64;
constexpr uint32_t bkt_slot_of(uint32_t q) { return (q % kBktGroupSize) * kBktGroups + q / kBktGroupSize; }
constexpr uint32_t bkt_group_last(uint32_t group) { return bkt_slot_of(group * kBktGroupSize + kBktGroupSize - 1); }
// groups: how many groups lie wholly at or below the key (their last bound <= key); inside: how many bounds of the next
// group do.  The bucket of a key is the number of bounds at or below it, minus one: t_0 is at or below every key.
constexpr uint32_t bkt_bucket_of(uint32_t groups, uint32_t inside) { return groups * kBktGroupSize + inside - 1u; }

} // namespace sots
