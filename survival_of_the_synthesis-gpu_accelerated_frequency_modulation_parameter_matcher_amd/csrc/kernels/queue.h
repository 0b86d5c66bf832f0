// queue.h -- the chunk queue's turnover: k_queue_turnover (best-ever record, stop rule, retirement and refill of a slot in
// one launch) and the k_fft_x target table it rewrites.
#pragma once
#include "common.h"
#include "objective.h"
#include "spectral_x.h"
#include "variation.h"
#include "../sots_stop_rule.h"

// contraction: off (the translation unit's default: the refill draws as k_init_population_seg does)
#pragma clang fp contract(off)
namespace sots { namespace {

// ------------------------------------------------------------------------------------
// Chunk queue (sots_batch_queue_run): the run record of k_track (best-ever only) and the TURNOVER in one launch, a
// workgroup per slot, after every generation's sort.  A slot whose chunk's stop rule holds at one of the chunk's own
// check boundaries - or whose counter has reached max_generations - stores the chunk's result, draws the next unstarted
// chunk (ONE returning atomic on the queue head; nothing else passes between workgroups inside the launch, kernel
// boundaries on the stream order the rest), and is re-initialised for it: rows as k_init_population_seg draws them,
// record cleared, counter zeroed, target table rewritten from the stored targets.  With the queue empty the slot goes idle.
// values / steps / fitness: the half the sort has just written (the turnover writes the new chunk's rows there: it is the
// half the next generation's variation reads).
// CARRY (sots_batch_queue_set_carry): the chunks are cut into segments of q.segment_chunks; the head counts
// SEGMENTS, and inside a segment the slot takes chunk + 1 without touching it.  Such a successor keeps the retired
// chunk's rows where they lie: row 0 becomes the best-ever record (the `rec` words threads 0..31 hold), rows 1..R-1 stay
// as the sort left them, and the refill draws rows R..P-1 only - by local row index, so they are a fresh start's rows.
// Without CARRY the body is the kernel's as it was before carrying existed.
// ------------------------------------------------------------------------------------
template <int LOG2N>
__device__ __forceinline__ void queue_fill_x_table(float *__restrict__ image, const float *__restrict__ target, uint32_t slot,
                                                   uint32_t t, uint32_t threads)
{
    float *table = image + kSegHead + (size_t)slot * x_seg_stride<LOG2N>();
    for (uint32_t le = t; le < (uint32_t)(kWave * x_points<LOG2N>()); le += threads) x_seg_target_entry<LOG2N>(table, target, le);
}

template <bool CARRY>
__global__ __launch_bounds__(256) void k_queue_turnover(float *__restrict__ values, float *__restrict__ steps, float *__restrict__ fitness,
                                                        PopDims pd, uint32_t *__restrict__ meta, float *__restrict__ rows, QueueArgs q,
                                                        uint32_t global_generation)
{
    __shared__ uint32_t next_s;
    const uint32_t c = blockIdx.x, t = threadIdx.x, threads = blockDim.x, p = pd.p, d = pd.d;
    uint32_t *slot = q.slot_table + 2u * (size_t)c;
    const uint32_t chunk = slot[0];
    if (chunk == kQueueNoChunk) return; // idle (uniform over the workgroup)
    const uint32_t g = slot[1] + 1u;    // the chunk's own counter after this generation
    float *v = values + (size_t)c * p * d, *s = steps + (size_t)c * p * d, *f = fitness + (size_t)c * p;
    uint32_t *m = meta + 2u * (size_t)c;
    float *row = rows + (size_t)kTrackRowFloats * c;

    // best-ever, as k_track: strictly better only
    const float f0 = f[0], old = __uint_as_float(m[0]);
    const bool wins = f0 < old;
    const float ever_f = wins ? f0 : old;
    const uint32_t ever_g = wins ? g : m[1];
    float rec = 0.0f; // thread t < kTrackRowFloats: word t of the record's row {values[16], steps[16]} after this generation
    if (t < kTrackRowFloats) {
        const uint32_t j = t % SOTS_MAX_DIMS;
        rec = wins && j < d ? (t < SOTS_MAX_DIMS ? v[j] : s[j]) : row[t];
    }
    const bool look = q.check_interval != 0u && g % q.check_interval == 0u;
    const bool retire = g >= q.max_generations || (look && stop_rule_holds(q.target_fitness, q.stall_generations, ever_f, ever_g, g));
    __syncthreads(); // every thread holds the slot's words and the old record before anybody replaces them
    if (!retire) {
        if (wins) {
            if (t < kTrackRowFloats) row[t] = rec;
            if (t == 0) {
                m[0] = __float_as_uint(f0);
                m[1] = g;
            }
        }
        if (t == 0) slot[1] = g;
        return;
    }

    // ---- retire: the result (sots_chunk_result), the kept population ----
    float *res = q.results + (size_t)chunk * kQueueResultFloats;
    if (t == 0) {
        reinterpret_cast<uint32_t *>(res)[0] = g;
        reinterpret_cast<uint32_t *>(res)[1] = ever_g;
        res[2] = ever_f;
        res[3] = f0;
    }
    if (t < kTrackRowFloats) res[4 + t] = rec;
    if (t < SOTS_MAX_DIMS) res[4 + kTrackRowFloats + t] = t < d ? v[t] : 0.0f;
    if (chunk == q.keep_chunk) {
        for (uint32_t e = t; e < p * d; e += threads) {
            q.kept_values[e] = v[e];
            q.kept_steps[e] = s[e];
        }
        for (uint32_t e = t; e < p; e += threads) q.kept_fitness[e] = f[e];
    }
    // a successor: the next chunk of this chunk's segment
    const bool successor = CARRY && queue_has_successor(chunk, q.segment_chunks, q.num_chunks);
    if (t == 0) {
        atomicAdd(&q.state[1], 1u);                    // retired
        atomicMax(&q.state[2], global_generation);     // the loop generation of the last retirement
        if (!CARRY) {
            next_s = atomicAdd(&q.state[0], 1u);       // the queue head: the next unstarted chunk
        } else if (successor) {
            next_s = chunk + 1u;                       // inside a segment the head is not touched
        } else {
            const uint32_t seg = atomicAdd(&q.state[0], 1u); // the queue head: the next unstarted SEGMENT
            next_s = queue_segment_start(seg, q.segment_chunks, q.num_segments, kQueueNoChunk);
        }
    }
    __syncthreads(); // the draw is in LDS, and the old rows have been read
    const uint32_t next = next_s;
    if (next >= q.num_chunks) {
        if (t == 0) slot[0] = kQueueNoChunk;
        return;
    }

    // ---- refill: k_init_population_seg's draws for chunk first_chunk + next, a cleared record, the target table ----
    uint32_t fresh = 0u; // the first element drawn: a successor's rows 0..R-1 are carried (R <= numParents <= p)
    if (CARRY && successor) {
        fresh = q.carry_rows * d;
        if (t < kTrackRowFloats) { // row 0: the retired chunk's best-ever record
            const uint32_t j = t % SOTS_MAX_DIMS;
            if (j < d) (t < SOTS_MAX_DIMS ? v : s)[j] = rec;
        }
        for (uint32_t i = t; i < q.carry_rows; i += threads) f[i] = 0.0f;
    }
    for (uint32_t e = fresh + t; e < p * d; e += threads) {
        const uint32_t i = e / d, gene = e - i * d;
        const U4 rn = philox4x32_10(pd.gid_base + i, q.first_chunk + next, gene >> 2, kTagInit, pd.seed_lo, pd.seed_hi);
        const float u = draw_unit(u4_at(rn, gene & 3u));
        s[e] = 0.1f;
        v[e] = (u < 0.0f) ? -u : u;
        if (gene == 0) f[i] = 0.0f;
    }
    if (t < kTrackRowFloats) row[t] = 0.0f;
    if (t == 0) {
        m[0] = 0x7F800000u;
        m[1] = 0u;
        slot[0] = next;
        slot[1] = 0u;
    }
    const float *tg = q.targets + (size_t)next * q.half_bins;
    switch (q.x_log2n) {
    case 8: queue_fill_x_table<8>(q.seg_image, tg, c, t, threads); break;
    case 11: queue_fill_x_table<11>(q.seg_image, tg, c, t, threads); break;
    case 12: queue_fill_x_table<12>(q.seg_image, tg, c, t, threads); break;
    case 13: queue_fill_x_table<13>(q.seg_image, tg, c, t, threads); break;
    default: { // k_fft / k_fft_big: the N/2 bins
        float *table = q.seg_image + kSegHead + (size_t)c * q.half_bins;
        for (uint32_t k = t; k < q.half_bins; k += threads) table[k] = tg[k];
    }
    }
}

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
