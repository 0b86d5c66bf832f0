// sots_kernels.h -- host-callable launchers of the gfx950 kernels (sots_kernels.hip).
// Internal to libsots_hip.so; the public boundary is include/sots_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/sots_hip.h"
#include "sots_rules.h" // MutateConsts

namespace sots {

constexpr uint32_t kWavetableSize = SOTS_WAVETABLE_SIZE;
constexpr uint32_t kTagInit = 0x494e4954u;   // PRNG domain words (4th Philox counter word)
constexpr uint32_t kTagMutate = 0x4d555441u;

struct SynthParams {
    float pmin[SOTS_MAX_DIMS];
    float pmax[SOTS_MAX_DIMS];
};

// Population geometry shared by most launches.
struct PopDims {
    uint32_t p;            // populationLength
    uint32_t d;            // numDimensions
    uint32_t num_parents;
    uint32_t block;        // recombination block (reference WRKGRPSIZE)
    uint32_t gid_base;
    uint32_t seed_lo, seed_hi;
    // recombine_source's divisions as shifts and masks where the sizes allow (they usually do: blocks of 32, 512 parent blocks)
    uint32_t block_shift;  // log2(block) when block is a power of two, else kNoPow2
    uint32_t npb;          // parent blocks: max(1, num_parents / block)
    uint32_t npb_mask;     // npb - 1 when npb is a power of two, else kNoPow2
    // rows 0 .. survivors-1 of the sorted half pass through variation as they are (make_gene, kernels/variation.h); a
    // setting of the context or batch (sots_set_survivors), 0 = the reference's strategy
    uint32_t survivors;
};
constexpr uint32_t kNoPow2 = 0xFFFFFFFFu;
inline PopDims make_pop_dims(uint32_t p, uint32_t d, uint32_t num_parents, uint32_t block, uint32_t gid_base, uint32_t seed_lo,
                             uint32_t seed_hi)
{
    PopDims pd{p, d, num_parents, block, gid_base, seed_lo, seed_hi, kNoPow2, 1u, kNoPow2, 0u};
    if (block && (block & (block - 1u)) == 0u)
        for (uint32_t sh = 0; sh < 32; ++sh)
            if ((1u << sh) == block) pd.block_shift = sh;
    pd.npb = block && num_parents / block ? num_parents / block : 1u;
    if ((pd.npb & (pd.npb - 1u)) == 0u) pd.npb_mask = pd.npb - 1u;
    return pd;
}

// Variation folded into the synthesis kernel (fused generation loop): when vin != nullptr every
// lane first builds its individual - recombination source rows of the current half, mutation -
// writes it to the other half and synthesises from it; with vin == nullptr the kernel reads
// `values` as is.
struct Variation {
    const float *vin, *sin; // current half (sorted)
    float *vout, *sout;     // other half
    PopDims pd;
    MutateConsts mc;
    uint32_t generation;
};

// Resident-workgroup counts of the persistent spectral kernels (occupancy queries), cached per
// CONTEXT: a context belongs to one device and is used from one thread at a time, so the cache
// needs no synchronisation (a process-wide cache would be shared by every device and thread).
struct OccCache {
    int fft[16], fitness[16], fused_win[16], fused_raw[16];
    int x_fft[16], x_fitness[16], x_fused_win[16], x_fused_raw[16], x_small[16];
    int wide[4]; // k_fft with twelve wavefronts per workgroup: spectrum writer, fused with / without window
    // device memory of the context: the fused long-row kernel's tables as they lie in LDS (launch_x_tables; null = the workgroups make them)
    const float *x_image;
};

// The objective of a spectral launch (sots_set_objective): SOTS_OBJECTIVE_MAGNITUDE, the reference's squared distance of
// the magnitudes, or SOTS_OBJECTIVE_LOG_MAGNITUDE, sum (ln(m + floor) - ln(t + floor))^2.  Under the log objective every
// target the launchers below are given - plain bins, table image, segmented image - holds ln(t + floor) instead of t:
// launch_objective_map makes the plain bins, the layouts are copied from them as they are from magnitudes.
// Per-bin weights (sots_set_objective_weights): F = sum_k (u_k e_k)^2 with e_k the signed error of the objective above and
// u_k = sqrt(w_k).  `weights` is u[N/2] on the device, plain bins (the staged fitness kernels read it); `weights_image` is
// the same table as the fused kernels read it (launch_weight_image: laid out as one chunk's target table).  Both null: no
// weights, and the launchers enqueue the unweighted kernels.
struct Objective {
    uint32_t kind = SOTS_OBJECTIVE_MAGNITUDE;
    float floor = 0.0f;
    const float *weights = nullptr;
    const float *weights_image = nullptr;
};
size_t weight_image_bytes(uint32_t log2n);
hipError_t launch_weight_image(hipStream_t st, float *image, const float *u, uint32_t log2n);
// dst[i] = ln(src[i] + floor) with the device routine the fitness epilogues apply to the candidate's bins
hipError_t launch_objective_map(hipStream_t st, float *dst, const float *src, size_t n, float floor);
// the cached occupancies belong to the kernels of one objective: forgotten when it changes (the image pointer stays)
inline void occ_forget(OccCache &oc)
{
    const float *image = oc.x_image;
    oc = OccCache{};
    oc.x_image = image;
}

// ---- variation ----
hipError_t launch_init_population(hipStream_t st, float *values, float *steps, float *fitness,
                                  const PopDims &pd, uint32_t chunk);
hipError_t launch_recombine(hipStream_t st, const float *vin, const float *sin, float *vout, float *sout,
                            const PopDims &pd);
hipError_t launch_mutate(hipStream_t st, float *values, float *steps, const PopDims &pd,
                         const MutateConsts &mc, uint32_t generation);
// recombine (in -> out) and mutate fused
hipError_t launch_recombine_mutate(hipStream_t st, const float *vin, const float *sin, float *vout,
                                   float *sout, const PopDims &pd, const MutateConsts &mc,
                                   uint32_t generation);

// ---- evaluation ----
// Small populations of the series voices: the synthesis kernel with the time axis in the lanes applies (it makes its own
// individuals from one thread per gene when given a Variation, whatever the number of genes)
bool synth_time_parallel(uint32_t kind, uint32_t p, uint32_t num_cus);
// ... and where the series voices run with the operators in the lanes (k_synth_ol: the workgroup makes its individuals too, a thread per gene)
bool synth_operators_in_lanes(uint32_t kind, uint32_t p, uint32_t num_cus);
// Audio rows are `pitch` floats apart (pitch >= N, a multiple of 4): a power-of-two row stride
// would put every lane of a row-per-lane store on the same memory channel.
// the voices with the arithmetic of the reference's device kernels (ocl_program.cl:280-443); no 4-op voice
hipError_t launch_synth_device_arith(hipStream_t st, uint32_t kind, const float *values, const float *wavetable, float *audio,
                                     const SynthParams &sp, uint32_t p, uint32_t log2n, uint32_t pitch);
hipError_t launch_synth(hipStream_t st, uint32_t kind, const float *values, const float *wavetable,
                        float *audio, const SynthParams &sp, uint32_t p, uint32_t log2n, uint32_t pitch,
                        uint32_t num_cus, const Variation *var = nullptr, bool allow_cut = true,
                        const sots_voice_graph *graph = nullptr, uint32_t waveforms = 0, const float *feedback = nullptr,
                        uint32_t feedback_genes = 0);
// SOTS_SYNTH_GRAPH (sots_synth_graph.hip): a checked graph (voice_graph_check), values[p][2 OPS]; it makes no individuals.
// waveforms: the operators' checked waveform codes, 3 bits each (pack_waveforms); 0, all sine, launches k_synth_graph,
// anything else its shaped sibling.  feedback: the operators' eight checked feedback indices (sots_set_voice_feedback) or
// null; any index other than 0 launches the feedback sibling, with the codes going through it too.  feedback_genes: the
// checked mask of sots_create_graph_genes; other than 0, values is [p][2 OPS + popcount] and the gene sibling is launched,
// with the codes and the fixed indices going through it; 0 launches exactly what is launched without it.  form: the handle's
// enum sots_graph_synth_form; graph_synth_form_for (sots_rules.h) says which kernel these p rows get - LANES launches
// exactly what was launched before there were forms, TIME_PARALLEL goes to launch_synth_graph_tp
hipError_t launch_synth_graph(hipStream_t st, const sots_voice_graph &graph, const float *values, const float *wavetable, float *audio,
                              const SynthParams &sp, uint32_t p, uint32_t log2n, uint32_t pitch, uint32_t num_cus, uint32_t waveforms = 0,
                              const float *feedback = nullptr, uint32_t feedback_genes = 0, uint32_t form = SOTS_GRAPH_FORM_LANES);
// ... its time-parallel form (sots_synth_graph_tp.hip): no feedback, no gene mask; any p (a CU's share beyond the plan's
// capacity is taken in several groups of rows)
hipError_t launch_synth_graph_tp(hipStream_t st, const sots_voice_graph &graph, const float *values, const float *wavetable, float *audio,
                                 const SynthParams &sp, uint32_t p, uint32_t log2n, uint32_t pitch, uint32_t num_cus, uint32_t waveforms);
hipError_t launch_window(hipStream_t st, float *audio, const float *window, uint32_t p, uint32_t log2n,
                         uint32_t pitch);
// audio[P][pitch] -> spectrum[P][N+8]
hipError_t launch_fft(hipStream_t st, const float *audio, float *spectrum, const float2 *twiddle,
                      uint32_t p, uint32_t log2n, uint32_t pitch, uint32_t num_cus, OccCache *occ);
// spectrum[P][N+8] x target[N/2] -> fitness[P]
hipError_t launch_fitness(hipStream_t st, const float *spectrum, const float *target, float *fitness,
                          uint32_t p, uint32_t log2n, float inv_n, float inv_wf, uint32_t num_cus, OccCache *occ,
                          const Objective &obj = Objective{});
// audio[P][pitch] (x window when window != nullptr) x target -> fitness[P]; no spectrum in memory
size_t x_table_bytes(uint32_t log2n);
hipError_t launch_x_tables(hipStream_t st, float *image, const float2 *twiddle, const float *window, const float *target, uint32_t log2n);
// List mode of the one-launch selection: the kernel that computes a row's fitness also files the row's key under its
// bucket between the splitters of `slot`, so that the selection reads its bucket from `lists` instead of streaming all
// P fitness values.  A bucket's list is kSelListShards segments of kSelListSeg places, each with a counter of its own:
// a filing workgroup uses the segment of its number (one word takes some 88 returning atomics per microsecond on this
// GPU, and a converged population sends the whole chip to three buckets at a time).  cnt: buckets x kSelListShards
// counters, ALL ZERO when the filling launch starts, which count every key of the closed buckets, also those their
// segment has no place for (the open last bucket is P minus their sum); lists: buckets x kSelListCap keys.
// cnt_other: the other counter set, which the consuming selection leaves zeroed for the next generation.
constexpr uint32_t kSelListCap = 2048, kSelListShards = 16, kSelListSeg = kSelListCap / kSelListShards;
constexpr uint32_t kSelListMaxBuckets = 256; // splitters per slot up to which keys can be filed (the bounds sit in LDS)
struct SelLists {
    const uint64_t *slot;
    uint32_t *cnt, *cnt_other;
    uint64_t *lists;
    uint32_t buckets;
};
// is there a bucketing kernel for this shape (the wide N = 1024 spectral kernel with the window, a slot that fits its LDS)?
bool select_lists_apply(uint32_t p, uint32_t log2n, uint32_t num_cus);
size_t select_lists_bytes(uint32_t num_cus);     // the key lists
size_t select_counters_bytes();                  // ONE counter set
// files the keys of fitness[0 .. p) as the bucketing spectral kernel would (tests: any fitness, any slot)
hipError_t launch_bucket_fitness(hipStream_t st, const float *fitness, uint32_t p, const SelLists &lists);
// lists: also file the keys (only where select_lists_apply(); elsewhere hipErrorInvalidValue)
hipError_t launch_fft_fitness(hipStream_t st, const float *audio, const float *window, const float *target,
                              float *fitness, const float2 *twiddle, uint32_t p, uint32_t log2n, uint32_t pitch,
                              float inv_n, float inv_wf, uint32_t num_cus, OccCache *occ, const SelLists *lists = nullptr,
                              const Objective &obj = Objective{});

// Island exchange folded into sortPopulation (one generation of the fused loop, set through
// sots_fuse_exchange_next_sort): the kernel that moves the sorted rows also
//   * takes destination rows [imm_first, imm_first + imm_rows) from `imm` (rows [fitness, values.., steps..] of an
//     all-gathered buffer, source rows [skip_first, skip_first + skip_count) - the island's own block - passed
//     over) instead of from the local population: sots_inject_gathered_device without its launch;
//   * copies the best `sink_rows` rows - immigrants included where the ranges overlap - to `sink` in the same row
//     format: sots_pack_elites_device without its launch.
// Either pointer may be null.
struct SortExchange {
    float *sink;
    const float *imm;
    uint32_t sink_rows, imm_first, imm_rows, skip_first, skip_count;
};

// ---- selection ----
// keys: sort_keys_bytes(P) bytes; scratch: sort_scratch_bytes(P) bytes.  Rows that would land in front of
// `first_row` are not written (the selection below has placed them already).
size_t sort_scratch_bytes(uint32_t p);
size_t sort_keys_bytes(uint32_t p);
hipError_t launch_sort(hipStream_t st, const float *vin, const float *sin, const float *fin,
                       float *vout, float *sout, float *fout, uint64_t *keys, void *scratch, uint32_t p,
                       uint32_t d, uint32_t first_row = 0, const SortExchange *exchange = nullptr);
// the best `need` rows in order into rows 0..need-1 of the out arrays, other rows untouched; only
// where select_applies() (otherwise hipErrorInvalidValue)
bool select_applies(uint32_t p, uint32_t need);
size_t select_scratch_bytes(uint32_t p); // the sort scratch must hold at least this much
hipError_t launch_select(hipStream_t st, const float *vin, const float *sin, const float *fin, float *vout,
                         float *sout, float *fout, uint64_t *keys, void *scratch, uint32_t p, uint32_t d, uint32_t need,
                         uint32_t num_cus, const SortExchange *exchange = nullptr);
// The same selection in ONE launch, ranked between the splitters of a slot (k_sel_splitters): spl_in holds
// select_splitter_count() 64-bit keys - ANY values give the exact rows, the previous generation's give them fast -
// and spl_out (a different slot) receives this population's.  keys: the sort_keys_bytes(P) buffer (a bucket that
// outgrows the LDS is ordered there).  launch_select_seed fills a slot from the sorted fitness launch_select wrote.
// lists (filled between the splitters of spl_in): a workgroup takes its bucket from them, and streams as without
// them only where its list overflowed or the open bucket has rows or splitters to place.
uint32_t select_splitter_count(uint32_t num_cus);
size_t select_splitter_slot_bytes();
hipError_t launch_select_splitters(hipStream_t st, const float *vin, const float *sin, const float *fin, float *vout,
                                   float *sout, float *fout, uint64_t *keys, const uint64_t *spl_in, uint64_t *spl_out,
                                   uint32_t p, uint32_t d, uint32_t need, uint32_t num_cus,
                                   const SortExchange *exchange = nullptr, const SelLists *lists = nullptr);
hipError_t launch_select_seed(hipStream_t st, const float *fsorted, uint64_t *spl_out, uint32_t need, uint32_t num_cus);

// ---- island exchange ----
hipError_t launch_pack_rows(hipStream_t st, const float *values, const float *steps, const float *fitness,
                            float *rows, uint32_t first_row, uint32_t n_rows, uint32_t d);
// source rows [skip_first, skip_first + skip_count) are passed over
hipError_t launch_unpack_rows(hipStream_t st, float *values, float *steps, float *fitness,
                              const float *rows, uint32_t first_row, uint32_t n_rows, uint32_t d,
                              uint32_t skip_first, uint32_t skip_count);

// ---- chunks in flight (sots_batch) ----
// `chunks` populations of pd.p rows, chunk-major (row r: chunk r / P, local index r % P); each chunk draws what a context
// of its own would (init: chunk first_chunk + c; variation: the local index)
hipError_t launch_init_population_seg(hipStream_t st, float *values, float *steps, float *fitness, const PopDims &pd,
                                      uint32_t first_chunk, uint32_t chunks);
hipError_t launch_recombine_mutate_seg(hipStream_t st, const float *vin, const float *sin, float *vout, float *sout,
                                       const PopDims &pd, const MutateConsts &mc, uint32_t generation, uint32_t chunks);
// Segmented target image: uint32 rows-per-chunk in word 0, chunk c's target table from float 64 + c * stride on (the N/2
// bins, or k_fft_x's per-(lane, register) table where that kernel runs).  The caller writes word 0 and zeroes the image
// once; launch_seg_targets fills the tables from targets[chunks][N/2] (device memory).
constexpr uint32_t kSegTargetHeadFloats = 64;
size_t seg_target_stride(uint32_t log2n);
size_t seg_target_bytes(uint32_t log2n, uint32_t chunks);
hipError_t launch_seg_targets(hipStream_t st, float *image, const float *targets, uint32_t log2n, uint32_t chunks);
// launch_fft_fitness (window applied) over rows of consecutive chunks, each row against its chunk's target
hipError_t launch_fft_fitness_seg(hipStream_t st, const float *audio, const float *window, const float *seg_image, float *fitness,
                                  const float2 *twiddle, uint32_t p, uint32_t log2n, uint32_t pitch, float inv_n, float inv_wf,
                                  uint32_t num_cus, OccCache *occ, const Objective &obj = Objective{});
// the whole-population sort of each chunk (P <= 1024: k_sort_small, a workgroup per chunk)
hipError_t launch_sort_seg(hipStream_t st, const float *vin, const float *sin, const float *fin, float *vout, float *sout,
                           float *fout, uint32_t p, uint32_t d, uint32_t chunks);

// ---- run record (sots_track / sots_batch_track) ----
// One launch, a workgroup per chunk, on the half a generation's sortPopulation has just written (rows chunk-major, p rows
// per chunk; a context is one chunk).  It reads rows 0..parents-1 only.
//   * best-ever: when fitness[0] is strictly below the chunk's recorded best (NaN never is), row 0 - values, steps,
//     fitness - and `generation` replace the record.  meta: uint32[chunks][2] = {fitness bits, generation};
//     rows: float[chunks][kTrackRowFloats] = {values[SOTS_MAX_DIMS], steps[SOTS_MAX_DIMS]}.
//   * history, when slot != kTrackNoSlot: one sots_gen_record into hist[chunk][slot] of float[chunks][capacity]
//     [kTrackRecordFloats].  The means are pairwise (tree) sums whose shape depends on `parents` and `d` alone: the same
//     rows give the same bits in any launch, whatever the number of chunks.  No atomics.
constexpr uint32_t kTrackRowFloats = 2 * SOTS_MAX_DIMS;
constexpr uint32_t kTrackRecordFloats = 24; // sizeof(sots_gen_record) / 4
constexpr uint32_t kTrackNoSlot = 0xFFFFFFFFu;
// every chunk's record: fitness +inf, generation 0, zeroed rows
hipError_t launch_track_clear(hipStream_t st, uint32_t *meta, float *rows, uint32_t chunks);
hipError_t launch_track(hipStream_t st, const float *values, const float *steps, const float *fitness, uint32_t p, uint32_t d,
                        uint32_t parents, uint32_t generation, uint32_t chunks, uint32_t *meta, float *rows, float *hist,
                        uint32_t capacity, uint32_t slot);

// ---- chunk queue (sots_batch_queue_run) ----
// M chunks go through `slots` slots of a batch; a slot runs its chunk under a generation counter of its own.  Device
// state: state = uint32[4] {queue head (next unstarted chunk), chunks retired, loop generation of the last retirement, 0};
// slot_table = uint32[slots][2] {chunk index or kQueueNoChunk, generations completed}; results = float[M]
// [kQueueResultFloats] (sots_chunk_result); targets = float[M][N/2]; kept_*: one chunk's current half as it was retired.
constexpr uint32_t kQueueNoChunk = 0xFFFFFFFFu;
constexpr uint32_t kQueueResultFloats = 4 + 3 * SOTS_MAX_DIMS; // sizeof(sots_chunk_result) / 4
struct QueueArgs {
    uint32_t *state, *slot_table;
    float *results;
    const float *targets;
    float *seg_image; // the batch's segmented target image: slot c's table is rewritten when the slot is refilled
    float *kept_values, *kept_steps, *kept_fitness;
    uint32_t num_chunks, first_chunk, max_generations, keep_chunk;
    uint32_t check_interval; // 0: no rule, every chunk runs max_generations
    float target_fitness;
    uint32_t stall_generations;
    uint32_t x_log2n;   // queue_x_log2n(): log2 N where the image holds k_fft_x's tables, 0 where it holds the N/2 bins
    uint32_t half_bins; // N/2
    // carry (sots_batch_queue_set_carry): carry_rows 0 = off, and the two words behind it are not read.  Otherwise 1 <=
    // carry_rows <= numParents, segment_chunks >= 1, num_segments = ceil(num_chunks / segment_chunks), and state[0] counts
    // segments: the next unstarted one
    uint32_t carry_rows, segment_chunks, num_segments;
};
uint32_t queue_x_log2n(uint32_t log2n);
// k_recombine_mutate_seg with the generation of row r's slot read from slot_table
hipError_t launch_recombine_mutate_queue(hipStream_t st, const float *vin, const float *sin, float *vout, float *sout, const PopDims &pd,
                                         const MutateConsts &mc, const uint32_t *slot_table, uint32_t slots);
// after a generation's sort, on the half it wrote: the best-ever record of every busy slot (meta, rows: as launch_track) and
// the turnover of those whose chunk ends here; global_generation = generations the queue loop has run, this one included.
// q.carry_rows chooses the kernel: 0, the turnover as it always was; otherwise its carry form
hipError_t launch_queue_turnover(hipStream_t st, float *values, float *steps, float *fitness, const PopDims &pd, uint32_t *meta,
                                 float *rows, const QueueArgs &q, uint32_t global_generation, uint32_t slots);

uint32_t next_pow2(uint32_t v);

} // namespace sots
