// sots_queue_host.cpp -- the host-only entry points of the chunk queue: no device, no handle, no HIP header, so that the
// sanitizer builds of tests/ compile this file as it stands (tests/test_chunk_queue_cpu.py).
#include "../../include/sots_hip.h"
#include "sots_stop_rule.h"

extern "C" int sots_queue_makespan(const uint32_t *generations_run, uint32_t num_chunks, uint32_t slots, uint64_t *global_generations)
{
    if (global_generations) *global_generations = 0;
    if (!global_generations || slots == 0 || (num_chunks && !generations_run)) return SOTS_ERR_INVALID;
    *global_generations = sots::queue_makespan(generations_run, num_chunks, slots);
    return SOTS_OK;
}
