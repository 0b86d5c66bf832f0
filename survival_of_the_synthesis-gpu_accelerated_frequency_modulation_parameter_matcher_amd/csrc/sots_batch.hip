// sots_batch.hip -- chunks in flight: the sots_batch_* entry points of include/sots_hip.h.  One handle advances C
// independent chunk populations, each against its own target, with the launches of ONE population per generation
// (variation | synthesis | window + FFT + fitness | sort, each over every chunk's rows).  Chunk c of a batch computes
// bit for bit what a sots_ctx of the same configuration computes for chunk first_chunk_index + c ("Chunks in
// flight").  No CPU fallback: every compute entry point launches gfx950 kernels or fails with an error code.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sots_hip.h"
#include "sots_analyse.h"
#include "sots_engine.h"
#include "sots_host_math.h"
#include "sots_kernels.h"
#include "sots_stop_rule.h"
#include "sots_track.h"

using namespace sots;

namespace {
thread_local std::string g_create_error; // (this file's: sots_batch_last_error(NULL))
constexpr uint32_t kBatchMaxPopulation = 1024; // one k_sort_small workgroup per chunk
constexpr uint64_t kQueueMaxTargetBytes = 1ull << 30; // the stored targets of a chunk queue (include/sots_hip.h)
static_assert(sizeof(sots_chunk_result) == 208 && sizeof(sots_chunk_result) == sots::kQueueResultFloats * sizeof(float),
              "sots_chunk_result is what k_queue_turnover writes");
} // namespace

struct sots_batch : sots::Engine {
    uint32_t max_chunks = 0, active = 0; // active: chunks of the last target call
    uint32_t rot = 0, generation = 0;
    // device buffers; rows chunk-major, max_chunks * P per rotation half
    float *values = nullptr, *steps = nullptr, *fitness = nullptr; // [2][C P][D], [2][C P][D], [2][C P]
    float *audio = nullptr;                                        // [C P][pitch]
    float *targets = nullptr;                                      // [C][N/2] as uploaded
    // the objective of every chunk (sots_batch_set_objective).  Under LOG_MAGNITUDE the segmented image is laid out from
    // targets_ln = ln(targets + floor) and the queue's turnover reads q_targets_ln, both made on the device from the
    // uploaded magnitudes (batch_derive / queue_derive) and allocated with the first log objective that needs them
    // The per-bin weights are one table for every chunk; the targets' images do not depend on it.
    float *targets_ln = nullptr;                                   // [C][N/2]
    float *seg_image = nullptr;                                    // segmented target image (sots_kernels.h)
    TrackState track{}; // run record of every chunk (sots_batch_track)
    // chunk queue (sots_batch_queue_*): the stored targets, the results, the kept population, the slot table
    uint32_t q_chunks = 0;           // chunks of the stored queue (0: none)
    bool q_ran = false, q_kept = false;
    float *q_targets = nullptr;      // [q_chunks][N/2]
    float *q_targets_ln = nullptr;   // [q_chunks][N/2], log objective only
    float *q_results = nullptr;      // [q_chunks][kQueueResultFloats]
    float *q_kept_rows = nullptr;    // values [P][D], steps [P][D], fitness [P]
    uint32_t *q_state = nullptr;     // {head, retired, last retirement, 0} and the slot table [max_chunks][2] behind them
    uint32_t *q_pinned = nullptr;    // host uint32[2][4]: the loop's look at q_state, one per block in flight
    hipEvent_t q_event[2] = {nullptr, nullptr};
    // carried rows (sots_batch_queue_set_carry): a setting of the handle, kept over targets and runs.  0, 0: off
    uint32_t q_carry_rows = 0, q_segment_chunks = 0;
    // analysis on the device (sots_batch_set_analysis): how the audio target calls make their spectra, and the scratch of
    // every device analysis (the uploaded signal, what sots_batch_analyse_audio_hop / _queue_score_audio_hop read back)
    uint32_t analysis = SOTS_ANALYSIS_HOST;
    AnalyseScratch an{};

    size_t rows() const { return (size_t)max_chunks * P; }
    float *val(uint32_t half) const { return values + (size_t)half * rows() * D; }
    float *stp(uint32_t half) const { return steps + (size_t)half * rows() * D; }
    float *fit(uint32_t half) const { return fitness + (size_t)half * rows(); }
};

namespace {

std::string &err_of(const sots_batch *b) { return b ? b->err : g_create_error; }

#define BATCH_REQUIRE(b) \
    do {                 \
        if (!(b)) return SOTS_FAIL(nullptr, SOTS_ERR_INVALID, "null batch"); \
    } while (0)

void queue_release(sots_batch *b)
{
    void *bufs[] = {b->q_targets, b->q_targets_ln, b->q_results, b->q_kept_rows, b->q_state};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    if (b->q_pinned) (void)hipHostFree(b->q_pinned);
    for (hipEvent_t &e : b->q_event)
        if (e) (void)hipEventDestroy(e), e = nullptr;
    b->q_targets = b->q_targets_ln = b->q_results = b->q_kept_rows = nullptr;
    b->q_state = b->q_pinned = nullptr;
    b->q_chunks = 0;
    b->q_ran = b->q_kept = false;
}

void free_batch(sots_batch *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    void *bufs[] = {b->values, b->steps, b->fitness, b->audio, b->targets, b->targets_ln, b->seg_image};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    track_release(b->track);
    analyse_release(b->an);
    queue_release(b);
    engine_release(*b);
    delete b;
}

// a creation that fails: its text outlives the handle in the thread's store
int abandon(sots_batch *b, int rc)
{
    g_create_error = b->err;
    free_batch(b);
    return rc;
}

bool log_objective(const sots_batch *b) { return b->obj.kind == SOTS_OBJECTIVE_LOG_MAGNITUDE; }

// the segmented target image of chunks 0 .. num_chunks-1 from b->targets under b->obj; every chunk's record starts over
int batch_derive(sots_batch *b, uint32_t num_chunks)
{
    const float *src = b->targets;
    if (log_objective(b)) {
        const size_t m = b->N / 2;
        if (!b->targets_ln) SOTS_HIP(b, hipMalloc((void **)&b->targets_ln, (size_t)b->max_chunks * m * sizeof(float)));
        SOTS_HIP(b, launch_objective_map(b->stream, b->targets_ln, b->targets, (size_t)num_chunks * m, b->obj.floor));
        src = b->targets_ln;
    }
    SOTS_HIP(b, launch_seg_targets(b->stream, b->seg_image, src, b->log2n, num_chunks));
    SOTS_HIP(b, track_clear(b->track, b->stream));
    SOTS_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

// the stored queue targets as the turnover copies them into the image: the magnitudes, or their log image
int queue_derive(sots_batch *b)
{
    if (b->q_chunks == 0 || !log_objective(b)) return SOTS_OK;
    const size_t n = (size_t)b->q_chunks * (b->N / 2);
    if (!b->q_targets_ln) SOTS_HIP(b, hipMalloc((void **)&b->q_targets_ln, n * sizeof(float)));
    SOTS_HIP(b, launch_objective_map(b->stream, b->q_targets_ln, b->q_targets, n, b->obj.floor));
    SOTS_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}
const float *queue_targets(const sots_batch *b) { return log_objective(b) ? b->q_targets_ln : b->q_targets; }

int require_active(const sots_batch *b)
{
    if (b->active == 0)
        return SOTS_FAIL(b, SOTS_ERR_STATE, "no target: call sots_batch_set_target_audio or sots_batch_set_target_spectra first");
    return SOTS_OK;
}

// num_chunks spectra of N/2 magnitudes from audio, chunk c from sample c * hop on: the single context's host transform,
// chunk by chunk
std::vector<float> spectra_at_hop(const sots_batch *b, const float *audio, uint32_t hop, uint32_t num_chunks)
{
    const uint32_t m = b->N / 2;
    std::vector<float> mag((size_t)num_chunks * m);
    for (uint32_t c = 0; c < num_chunks; ++c) {
        const std::vector<float> one = target_spectrum(audio + (size_t)c * hop, b->N, b->window64, b->window_factor);
        memcpy(mag.data() + (size_t)c * m, one.data(), (size_t)m * sizeof(float));
    }
    return mag;
}

// The device analysis, enqueued: the samples of `frames` frames at a hop go up into the batch's scratch, once, and their
// magnitudes (bins: the scaled bins, for launch_score_frames) are written to dst, device memory.  The caller has checked
// the counts (analysis_frames_check) and synchronises before `audio` may go away.
int analyse_to(sots_batch *b, const float *audio, uint32_t hop, uint32_t frames, float *dst, bool bins)
{
    const size_t need = (size_t)analysis_samples(frames, hop, b->N);
    SOTS_HIP(b, analyse_reserve(b->an, need, 0, 0));
    SOTS_HIP(b, hipMemcpyAsync(b->an.signal, audio, need * sizeof(float), hipMemcpyHostToDevice, b->stream));
    SOTS_HIP(b, launch_analyse(b->stream, b->an.signal, b->window, b->twiddle, dst, bins, b->log2n, hop, frames, b->inv_n, b->inv_wf));
    return SOTS_OK;
}
bool device_analysis(const sots_batch *b) { return b->analysis == SOTS_ANALYSIS_DEVICE; }
// the audio target calls under SOTS_ANALYSIS_DEVICE: one upload holds at most kAnalysisMaxSamples
int device_samples_check(const sots_batch *b, uint64_t need)
{
    if (need > kAnalysisMaxSamples)
        return SOTS_FAIL(b, SOTS_ERR_INVALID, "device analysis: %llu samples of target audio, more than %llu", (unsigned long long)need,
                         (unsigned long long)kAnalysisMaxSamples);
    return SOTS_OK;
}

// One generation of `chunks` chunk populations, enqueued: variation | synthesis | window + FFT + fitness | sort, each
// over every chunk's rows, and the rotation index back where the sorted rows are.  vary(src, dst) launches the
// variation, the caller's own: by the batch's generation counter, or by the queue's slot table.
template <class Vary> int enqueue_generation(sots_batch *b, uint32_t chunks, Vary vary)
{
    const uint32_t rows = chunks * b->P;
    // recombine + mutate, current half -> other half
    uint32_t src = b->rot, dst = b->rot ^ 1u;
    SOTS_HIP(b, vary(src, dst));
    b->rot = dst;
    // synthesis: per row, so the single context's launcher serves every chunk's rows at once
    SOTS_HIP(b, engine_synthesise(*b, b->val(b->rot), b->audio, rows, nullptr, true));
    // window + FFT + fitness, every row against its chunk's target
    SOTS_HIP(b, launch_fft_fitness_seg(b->stream, b->audio, b->window, b->seg_image, b->fit(b->rot), b->twiddle, rows, b->log2n,
                                       b->pitch, b->inv_n, b->inv_wf, b->num_cus, &b->occ, b->obj));
    // sortPopulation of every chunk (whole population: P <= 1024), current half -> other half
    src = b->rot, dst = b->rot ^ 1u;
    SOTS_HIP(b, launch_sort_seg(b->stream, b->val(src), b->stp(src), b->fit(src), b->val(dst), b->stp(dst), b->fit(dst), b->P,
                                b->D, chunks));
    b->rot = dst;
    return SOTS_OK;
}

// A new stored queue of num_chunks chunks (the caller has checked the count against kQueueMaxTargetBytes): an earlier
// queue is released, the buffers are allocated, fill() enqueues what writes b->q_targets - the copy of uploaded
// magnitudes, or the device analysis - and the targets' derived table follows.
template <class Fill> int queue_store(sots_batch *b, uint32_t num_chunks, Fill fill)
{
    const uint64_t need = (uint64_t)num_chunks * (b->N / 2);
    if (int rc = engine_bind(*b)) return rc;
    SOTS_HIP(b, hipStreamSynchronize(b->stream));
    queue_release(b);
    const size_t pd_floats = (size_t)b->P * b->D;
#define QUEUE_HIP(call) SOTS_HIP_OR(b, call, queue_release(b); return rc_)
    QUEUE_HIP(hipMalloc((void **)&b->q_targets, need * sizeof(float)));
    QUEUE_HIP(hipMalloc((void **)&b->q_results, (size_t)num_chunks * sizeof(sots_chunk_result)));
    QUEUE_HIP(hipMalloc((void **)&b->q_kept_rows, (2 * pd_floats + b->P) * sizeof(float)));
    QUEUE_HIP(hipMalloc((void **)&b->q_state, (4 + 2 * (size_t)b->max_chunks) * sizeof(uint32_t)));
    QUEUE_HIP(hipHostMalloc((void **)&b->q_pinned, 2 * 4 * sizeof(uint32_t), hipHostMallocDefault));
    for (hipEvent_t &e : b->q_event) QUEUE_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (int rc = fill()) {
        queue_release(b);
        return rc;
    }
    QUEUE_HIP(hipStreamSynchronize(b->stream));
#undef QUEUE_HIP
    b->q_chunks = num_chunks;
    if (int rc = queue_derive(b)) {
        queue_release(b);
        return rc;
    }
    return SOTS_OK;
}

} // namespace

extern "C" {

// sots_batch_create (graph == nullptr), sots_batch_create_graph (feedback_genes == 0) and sots_batch_create_graph_genes
static int create_batch(const sots_config *cfg, const sots_voice_graph *graph, uint32_t feedback_genes, uint32_t max_chunks, sots_batch **out)
{
    *out = nullptr;
    // the configuration first, then the batch's own limits: a machine without a GPU still tells a bad one from a good one
    SOTS_REFUSE(nullptr, config_check(*cfg, kNoPopulationLimit, graph, feedback_genes));
    const uint64_t p64 = (uint64_t)cfg->num_parents + cfg->num_offspring;
    if (p64 > kBatchMaxPopulation)
        return SOTS_FAIL(nullptr, SOTS_ERR_INVALID, "a batch takes chunk populations of at most %u, got %llu (larger ones fill the GPU alone: sots_create)",
                     kBatchMaxPopulation, (unsigned long long)p64);
    if (max_chunks == 0) return SOTS_FAIL(nullptr, SOTS_ERR_INVALID, "max_chunks must be at least 1");
    if ((uint64_t)max_chunks * p64 > (1ull << 26))
        return SOTS_FAIL(nullptr, SOTS_ERR_INVALID, "max_chunks %u x population %llu exceeds 2^26 rows", max_chunks, (unsigned long long)p64);

    sots_batch *b = new sots_batch();
    if (int rc = engine_create(*b, *cfg, graph, 32, feedback_genes)) return abandon(b, rc); // (the pad of sots_create: rows off the power-of-two stride)
    b->max_chunks = max_chunks;
#define CREATE_HIP(call) SOTS_HIP_OR(b, call, return abandon(b, rc_))
    const size_t pd_bytes = (size_t)2 * b->rows() * b->D * sizeof(float);
    const size_t audio_bytes = b->rows() * b->pitch * sizeof(float);
    const size_t targets_bytes = (size_t)max_chunks * (b->N / 2) * sizeof(float);
    const size_t image_bytes = seg_target_bytes(b->log2n, max_chunks);
    CREATE_HIP(hipMalloc((void **)&b->values, pd_bytes));
    CREATE_HIP(hipMalloc((void **)&b->steps, pd_bytes));
    CREATE_HIP(hipMalloc((void **)&b->fitness, (size_t)2 * b->rows() * sizeof(float)));
    CREATE_HIP(hipMalloc((void **)&b->audio, audio_bytes));
    CREATE_HIP(hipMalloc((void **)&b->targets, targets_bytes));
    CREATE_HIP(hipMalloc((void **)&b->seg_image, image_bytes));
    CREATE_HIP(hipMemsetAsync(b->values, 0, pd_bytes, b->stream));
    CREATE_HIP(hipMemsetAsync(b->steps, 0, pd_bytes, b->stream));
    CREATE_HIP(hipMemsetAsync(b->fitness, 0, (size_t)2 * b->rows() * sizeof(float), b->stream));
    CREATE_HIP(hipMemsetAsync(b->audio, 0, audio_bytes, b->stream));
    CREATE_HIP(hipMemsetAsync(b->targets, 0, targets_bytes, b->stream));
    CREATE_HIP(hipMemsetAsync(b->seg_image, 0, image_bytes, b->stream));
    TableStaging staging;
    if (int rc = engine_upload_tables(*b, staging)) return abandon(b, rc);
    const uint32_t head = b->P; // the segmented image's word 0: rows per chunk
    CREATE_HIP(hipMemcpyAsync(b->seg_image, &head, sizeof head, hipMemcpyHostToDevice, b->stream));
    // k_fft_x's chunk-independent tables (twiddles, window); their target part is not read by the segmented kernels
    if (b->x_image) {
        CREATE_HIP(launch_x_tables(b->stream, b->x_image, b->twiddle, b->window, b->targets, b->log2n));
        b->occ.x_image = b->x_image;
    }
    CREATE_HIP(hipStreamSynchronize(b->stream));
#undef CREATE_HIP
    *out = b;
    return SOTS_OK;
}

int sots_batch_create(const sots_config *cfg, uint32_t max_chunks, sots_batch **out)
{
    if (!cfg || !out) return SOTS_FAIL(nullptr, SOTS_ERR_INVALID, "sots_batch_create: null argument");
    return create_batch(cfg, nullptr, 0, max_chunks, out);
}

int sots_batch_create_graph(const sots_config *cfg, const sots_voice_graph *graph, uint32_t max_chunks, sots_batch **out)
{
    if (!cfg || !graph || !out) return SOTS_FAIL(nullptr, SOTS_ERR_INVALID, "sots_batch_create_graph: null argument");
    return create_batch(cfg, graph, 0, max_chunks, out);
}

int sots_batch_create_graph_genes(const sots_config *cfg, const sots_voice_graph *graph, uint32_t feedback_genes, uint32_t max_chunks,
                                  sots_batch **out)
{
    if (!cfg || !graph || !out) return SOTS_FAIL(nullptr, SOTS_ERR_INVALID, "sots_batch_create_graph_genes: null argument");
    return create_batch(cfg, graph, feedback_genes, max_chunks, out);
}

int sots_batch_get_voice_feedback_genes(const sots_batch *b, uint32_t *feedback_genes)
{
    BATCH_REQUIRE(b);
    return engine_get_voice_feedback_genes(*b, feedback_genes);
}

int sots_batch_set_graph_synth_form(sots_batch *b, uint32_t form)
{
    BATCH_REQUIRE(b);
    return engine_set_graph_synth_form(*b, form);
}

int sots_batch_get_graph_synth_form(const sots_batch *b, uint32_t *requested, uint32_t *effective)
{
    BATCH_REQUIRE(b);
    return engine_get_graph_synth_form(*b, b->rows(), requested, effective);
}

void sots_batch_destroy(sots_batch *b) { free_batch(b); }

const char *sots_batch_last_error(const sots_batch *b) { return err_of(b).c_str(); }

int sots_batch_synchronize(sots_batch *b)
{
    BATCH_REQUIRE(b);
    if (int rc = engine_bind(*b)) return rc;
    SOTS_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

int sots_batch_set_target_spectra(sots_batch *b, const float *magnitudes, uint32_t num_bins, uint32_t num_chunks)
{
    BATCH_REQUIRE(b);
    if (num_chunks == 0 || num_chunks > b->max_chunks)
        return SOTS_FAIL(b, SOTS_ERR_INVALID, "num_chunks %u outside 1..%u", num_chunks, b->max_chunks);
    const uint64_t need = (uint64_t)num_chunks * (b->N / 2);
    if (!magnitudes || num_bins != need)
        return SOTS_FAIL(b, SOTS_ERR_SIZE, "%u target spectra need %llu bins, got %u", num_chunks, (unsigned long long)need, num_bins);
    if (int rc = engine_bind(*b)) return rc;
    SOTS_HIP(b, hipMemcpyAsync(b->targets, magnitudes, need * sizeof(float), hipMemcpyHostToDevice, b->stream));
    if (int rc = batch_derive(b, num_chunks)) return rc; // (new targets: every chunk's record starts over)
    b->active = num_chunks;
    return SOTS_OK;
}

int sots_batch_set_target_audio_hop(sots_batch *b, const float *audio, uint32_t num_samples, uint32_t hop, uint32_t num_chunks)
{
    BATCH_REQUIRE(b);
    if (num_chunks == 0 || num_chunks > b->max_chunks)
        return SOTS_FAIL(b, SOTS_ERR_INVALID, "num_chunks %u outside 1..%u", num_chunks, b->max_chunks);
    if (hop == 0 || hop > b->N) return SOTS_FAIL(b, SOTS_ERR_INVALID, "hop %u outside 1..%u", hop, b->N);
    const uint64_t need = (uint64_t)(num_chunks - 1u) * hop + b->N; // (hop = N: num_chunks * N)
    if (!audio || (uint64_t)num_samples < need)
        return SOTS_FAIL(b, SOTS_ERR_SIZE, "%u chunks of target audio need %llu samples, got %u", num_chunks, (unsigned long long)need, num_samples);
    if (device_analysis(b)) { // one upload, the spectra made where they are stored, then as sots_batch_set_target_spectra goes on
        if (int rc = device_samples_check(b, need)) return rc;
        if (int rc = engine_bind(*b)) return rc;
        if (int rc = analyse_to(b, audio, hop, num_chunks, b->targets, false)) return rc;
        if (int rc = batch_derive(b, num_chunks)) return rc; // (new targets: every chunk's record starts over)
        b->active = num_chunks;
        return SOTS_OK;
    }
    const std::vector<float> mag = spectra_at_hop(b, audio, hop, num_chunks);
    return sots_batch_set_target_spectra(b, mag.data(), (uint32_t)mag.size(), num_chunks);
}

int sots_batch_set_target_audio(sots_batch *b, const float *audio, uint32_t num_samples, uint32_t num_chunks)
{
    BATCH_REQUIRE(b);
    return sots_batch_set_target_audio_hop(b, audio, num_samples, b->N, num_chunks);
}

int sots_batch_init_population(sots_batch *b, uint32_t first_chunk_index)
{
    BATCH_REQUIRE(b);
    if (int rc = require_active(b)) return rc;
    if (int rc = engine_bind(*b)) return rc;
    b->rot = 0;
    b->generation = 0;
    SOTS_HIP(b, track_clear(b->track, b->stream));
    SOTS_HIP(b, launch_init_population_seg(b->stream, b->val(0), b->stp(0), b->fit(0), b->pd, first_chunk_index, b->active));
    return SOTS_OK;
}

int sots_batch_set_synth_arithmetic(sots_batch *b, uint32_t arith)
{
    BATCH_REQUIRE(b);
    return engine_set_synth_arithmetic(*b, arith);
}

int sots_batch_set_survivors(sots_batch *b, uint32_t n)
{
    BATCH_REQUIRE(b);
    return engine_set_survivors(*b, n);
}

int sots_batch_set_objective(sots_batch *b, uint32_t objective, float floor)
{
    BATCH_REQUIRE(b);
    Objective old;
    if (int rc = engine_set_objective(*b, objective, floor, &old)) return rc;
    int rc = b->active ? batch_derive(b, b->active) : SOTS_OK;
    if (rc == SOTS_OK) rc = queue_derive(b);
    if (rc != SOTS_OK) engine_restore_objective(*b, old), b->active = 0; // (the image may be half made: the ordinary calls need their targets again)
    return rc;
}

int sots_batch_set_objective_weights(sots_batch *b, const float *weights, uint32_t num_bins)
{
    BATCH_REQUIRE(b);
    Objective old;
    if (int rc = engine_set_objective_weights(*b, weights, num_bins, &old)) return rc;
    // (the targets' images stay; what the chunks had found under the old weights says nothing: every record starts over)
    SOTS_HIP_OR(b, track_clear(b->track, b->stream), engine_restore_objective(*b, old); return rc_);
    SOTS_HIP_OR(b, hipStreamSynchronize(b->stream), engine_restore_objective(*b, old); return rc_);
    return SOTS_OK;
}

// one setting for all chunks, active and queued; what the chunks had found with the old voice says nothing
int sots_batch_set_voice_waveforms(sots_batch *b, const uint32_t *codes, uint32_t count)
{
    BATCH_REQUIRE(b);
    SOTS_REFUSE(b, voice_waveforms_check(b->cfg.synth_kind, b->graph.num_operators, codes, count));
    if (int rc = engine_bind(*b)) return rc;
    SOTS_HIP(b, track_clear(b->track, b->stream));
    SOTS_HIP(b, hipStreamSynchronize(b->stream));
    return engine_set_voice_waveforms(*b, codes, count);
}

int sots_batch_get_voice_waveforms(const sots_batch *b, uint32_t codes[8])
{
    BATCH_REQUIRE(b);
    return engine_get_voice_waveforms(*b, codes);
}

int sots_batch_set_voice_feedback(sots_batch *b, const float *index, uint32_t count)
{
    BATCH_REQUIRE(b);
    SOTS_REFUSE(b, voice_feedback_check(b->cfg.synth_kind, b->graph.num_operators, index, count, b->feedback_genes));
    if (int rc = engine_bind(*b)) return rc;
    SOTS_HIP(b, track_clear(b->track, b->stream));
    SOTS_HIP(b, hipStreamSynchronize(b->stream));
    return engine_set_voice_feedback(*b, index, count);
}

int sots_batch_get_voice_feedback(const sots_batch *b, float index[8])
{
    BATCH_REQUIRE(b);
    return engine_get_voice_feedback(*b, index);
}

int sots_batch_execute_generations(sots_batch *b, uint32_t n)
{
    BATCH_REQUIRE(b);
    if (int rc = require_active(b)) return rc;
    if (int rc = engine_bind(*b)) return rc;
    for (uint32_t g = 0; g < n; ++g) {
        if (int rc = enqueue_generation(b, b->active, [b](uint32_t src, uint32_t dst) {
                return launch_recombine_mutate_seg(b->stream, b->val(src), b->stp(src), b->val(dst), b->stp(dst), b->pd, b->mc, b->generation,
                                                   b->active);
            }))
            return rc;
        b->generation += 1;
        // the run record of every active chunk (nothing when tracking is off)
        SOTS_HIP(b, track_record(b->track, b->stream, b->val(b->rot), b->stp(b->rot), b->fit(b->rot), b->P, b->D, b->cfg.num_parents,
                                 b->generation, b->active));
    }
    return SOTS_OK;
}

// ---- run record: as sots_track and its readers, per chunk ----
int sots_batch_track(sots_batch *b, uint32_t flags, uint32_t history_every, uint32_t history_capacity)
{
    BATCH_REQUIRE(b);
    SOTS_REFUSE(b, track_args_check(&flags, history_every, history_capacity, b->max_chunks));
    if (int rc = engine_bind(*b)) return rc;
    SOTS_HIP(b, hipStreamSynchronize(b->stream)); // a record launch may still be using the old buffers
    SOTS_HIP(b, track_setup(b->track, flags, history_every, history_capacity, b->max_chunks, b->stream));
    SOTS_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

int sots_batch_read_best_ever(sots_batch *b, float *values, size_t values_bytes, float *steps, size_t steps_bytes, float *fitness,
                              size_t fitness_bytes, uint32_t *generation, size_t generation_bytes)
{
    BATCH_REQUIRE(b);
    if (int rc = require_active(b)) return rc;
    if (!b->track.best_ever()) return SOTS_FAIL(b, SOTS_ERR_STATE, "best-ever tracking is off: call sots_batch_track first");
    const size_t d_bytes = (size_t)b->D * sizeof(float), v_bytes = b->active * d_bytes, f_bytes = (size_t)b->active * sizeof(float);
    if ((values && values_bytes != v_bytes) || (steps && steps_bytes != v_bytes) || (fitness && fitness_bytes != f_bytes) ||
        (generation && generation_bytes != f_bytes))
        return SOTS_FAIL(b, SOTS_ERR_SIZE, "best-ever byte counts must be %zu (values, steps) and %zu (fitness, generation)", v_bytes, f_bytes);
    if (int rc = engine_bind(*b)) return rc;
    const size_t pitch = (size_t)kTrackRowFloats * sizeof(float);
    if (values)
        SOTS_HIP(b, hipMemcpy2DAsync(values, d_bytes, b->track.rows, pitch, d_bytes, b->active, hipMemcpyDeviceToHost, b->stream));
    if (steps)
        SOTS_HIP(b, hipMemcpy2DAsync(steps, d_bytes, b->track.rows + SOTS_MAX_DIMS, pitch, d_bytes, b->active, hipMemcpyDeviceToHost, b->stream));
    SOTS_HIP(b, track_fetch_meta(b->track, b->stream, b->active));
    for (uint32_t c = 0; c < b->active; ++c) {
        if (fitness) fitness[c] = track_fitness(b->track, c);
        if (generation) generation[c] = b->track.pinned[2 * c + 1];
    }
    return SOTS_OK;
}

int sots_batch_read_history(sots_batch *b, uint32_t chunk, sots_gen_record *out, uint32_t capacity, uint32_t *written, uint64_t *taken)
{
    BATCH_REQUIRE(b);
    if (!b->track.history()) return SOTS_FAIL(b, SOTS_ERR_STATE, "the history is off: call sots_batch_track with SOTS_TRACK_HISTORY first");
    if (int rc = require_active(b)) return rc;
    if (chunk >= b->active) return SOTS_FAIL(b, SOTS_ERR_INVALID, "chunk %u not in 0..%u", chunk, b->active - 1);
    if (!written || (capacity && !out)) return SOTS_FAIL(b, SOTS_ERR_INVALID, "read_history: null argument");
    if (int rc = engine_bind(*b)) return rc;
    SOTS_HIP(b, track_read_history(b->track, b->stream, chunk, out, capacity, written));
    if (taken) *taken = b->track.taken;
    return SOTS_OK;
}

int sots_batch_execute_until(sots_batch *b, uint32_t max_generations, const sots_stop_rule *rule, uint32_t *generations_run)
{
    BATCH_REQUIRE(b);
    if (generations_run) *generations_run = 0;
    if (stop_rule_check(rule)) return SOTS_FAIL(b, SOTS_ERR_INVALID, "stop rule: null, wrong struct_size or check_interval 0");
    if (!b->track.best_ever()) return SOTS_FAIL(b, SOTS_ERR_STATE, "sots_batch_execute_until needs best-ever tracking: call sots_batch_track first");
    if (int rc = require_active(b)) return rc;
    uint32_t done = 0;
    while (done < max_generations) {
        const uint32_t block = rule->check_interval < max_generations - done ? rule->check_interval : max_generations - done;
        if (int rc = sots_batch_execute_generations(b, block)) return rc;
        done += block;
        if (generations_run) *generations_run = done;
        SOTS_HIP(b, track_fetch_meta(b->track, b->stream, b->active));
        bool all = true; // the chunks advance together: the batch is done when every chunk is
        for (uint32_t c = 0; c < b->active && all; ++c)
            all = sots_stop_rule_holds(rule, track_fitness(b->track, c), b->track.pinned[2 * c + 1], b->generation) == 1;
        if (all) break;
    }
    return SOTS_OK;
}

// ---- chunk queue: M chunks through the handle's slots, a slot refilled when its chunk's stop rule holds ----
int sots_batch_queue_targets_spectra(sots_batch *b, const float *magnitudes, uint64_t num_bins, uint32_t num_chunks)
{
    // (what needs no handle is checked first: a machine without a GPU still tells a bad call from a good one)
    if (num_chunks == 0) return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_batch_queue_targets: num_chunks must be at least 1");
    BATCH_REQUIRE(b);
    const uint64_t m = b->N / 2, need = (uint64_t)num_chunks * m;
    if (need * sizeof(float) > kQueueMaxTargetBytes)
        return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_batch_queue_targets: %u chunks of %llu bins exceed %llu bytes of stored targets", num_chunks,
                     (unsigned long long)m, (unsigned long long)kQueueMaxTargetBytes);
    if (!magnitudes || num_bins != need)
        return SOTS_FAIL(b, SOTS_ERR_SIZE, "%u queued target spectra need %llu bins, got %llu", num_chunks, (unsigned long long)need,
                     (unsigned long long)num_bins);
    return queue_store(b, num_chunks, [&]() -> int {
        SOTS_HIP(b, hipMemcpyAsync(b->q_targets, magnitudes, need * sizeof(float), hipMemcpyHostToDevice, b->stream));
        return SOTS_OK;
    });
}

int sots_batch_queue_targets_audio_hop(sots_batch *b, const float *audio, uint64_t num_samples, uint32_t hop, uint32_t num_chunks)
{
    // (what needs no handle is checked first: a machine without a GPU still tells a bad call from a good one)
    if (num_chunks == 0) return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_batch_queue_targets: num_chunks must be at least 1");
    BATCH_REQUIRE(b);
    const uint64_t m = b->N / 2;
    if ((uint64_t)num_chunks * m * sizeof(float) > kQueueMaxTargetBytes)
        return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_batch_queue_targets: %u chunks of %llu bins exceed %llu bytes of stored targets", num_chunks,
                     (unsigned long long)m, (unsigned long long)kQueueMaxTargetBytes);
    if (hop == 0 || hop > b->N) return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_batch_queue_targets: hop %u outside 1..%u", hop, b->N);
    const uint64_t need = (uint64_t)(num_chunks - 1u) * hop + b->N; // (hop = N: num_chunks * N)
    if (!audio || num_samples < need)
        return SOTS_FAIL(b, SOTS_ERR_SIZE, "%u queued chunks of target audio need %llu samples, got %llu", num_chunks,
                     (unsigned long long)need, (unsigned long long)num_samples);
    if (device_analysis(b)) { // one upload, the spectra made where they are stored, then as sots_batch_queue_targets_spectra goes on
        if (int rc = device_samples_check(b, need)) return rc;
        return queue_store(b, num_chunks, [&]() -> int { return analyse_to(b, audio, hop, num_chunks, b->q_targets, false); });
    }
    const std::vector<float> mag = spectra_at_hop(b, audio, hop, num_chunks);
    return sots_batch_queue_targets_spectra(b, mag.data(), mag.size(), num_chunks);
}

int sots_batch_queue_targets_audio(sots_batch *b, const float *audio, uint64_t num_samples, uint32_t num_chunks)
{
    // (what needs no handle is checked first: a machine without a GPU still tells a bad call from a good one)
    if (num_chunks == 0) return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_batch_queue_targets: num_chunks must be at least 1");
    BATCH_REQUIRE(b);
    return sots_batch_queue_targets_audio_hop(b, audio, num_samples, b->N, num_chunks);
}

// ---- analysis on the device ----
int sots_batch_set_analysis(sots_batch *b, uint32_t mode)
{
    BATCH_REQUIRE(b);
    SOTS_REFUSE(b, analysis_mode_check(mode));
    b->analysis = mode;
    return SOTS_OK;
}

int sots_batch_get_analysis(const sots_batch *b, uint32_t *mode)
{
    BATCH_REQUIRE(b);
    if (!mode) return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_batch_get_analysis: null pointer");
    *mode = b->analysis;
    return SOTS_OK;
}

int sots_batch_analyse_audio_hop(sots_batch *b, const float *audio, uint64_t num_samples, uint32_t hop, uint32_t num_frames, float *magnitudes,
                                 uint64_t num_bins)
{
    BATCH_REQUIRE(b);
    SOTS_REFUSE(b, analysis_frames_check("sots_batch_analyse_audio_hop", audio, num_samples, hop, num_frames, magnitudes, b->N));
    const uint64_t bins = (uint64_t)num_frames * (b->N / 2);
    if (num_bins != bins)
        return SOTS_FAIL(b, SOTS_ERR_SIZE, "sots_batch_analyse_audio_hop: %u frames give %llu bins, got room for %llu", num_frames,
                         (unsigned long long)bins, (unsigned long long)num_bins);
    if (int rc = engine_bind(*b)) return rc;
    SOTS_HIP(b, analyse_reserve(b->an, 0, (size_t)bins, 0));
    if (int rc = analyse_to(b, audio, hop, num_frames, b->an.out, false)) return rc;
    SOTS_HIP(b, hipMemcpyAsync(magnitudes, b->an.out, (size_t)bins * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    SOTS_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

int sots_batch_queue_score_audio_hop(sots_batch *b, const float *audio, uint64_t num_samples, uint32_t hop, float *fitness, uint32_t num_chunks)
{
    BATCH_REQUIRE(b);
    SOTS_REFUSE(b, analysis_frames_check("sots_batch_queue_score_audio_hop", audio, num_samples, hop, num_chunks, fitness, b->N));
    if (b->q_chunks == 0)
        return SOTS_FAIL(b, SOTS_ERR_STATE, "no queue: call sots_batch_queue_targets_audio or sots_batch_queue_targets_spectra first");
    if (num_chunks != b->q_chunks)
        return SOTS_FAIL(b, SOTS_ERR_SIZE, "sots_batch_queue_score_audio_hop: the queue holds %u chunks, got %u", b->q_chunks, num_chunks);
    if (int rc = engine_bind(*b)) return rc;
    // the scaled bins of every frame (two floats a bin), then one wavefront per frame against the stored target of its index
    SOTS_HIP(b, analyse_reserve(b->an, 0, (size_t)num_chunks * b->N, num_chunks));
    if (int rc = analyse_to(b, audio, hop, num_chunks, b->an.out, true)) return rc;
    SOTS_HIP(b, launch_score_frames(b->stream, reinterpret_cast<const float2 *>(b->an.out), queue_targets(b), b->an.fitness, b->log2n, num_chunks,
                                    b->obj));
    SOTS_HIP(b, hipMemcpyAsync(fitness, b->an.fitness, (size_t)num_chunks * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    SOTS_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

int sots_batch_queue_run(sots_batch *b, uint32_t first_chunk_index, uint32_t max_generations, const sots_stop_rule *rule,
                         uint32_t keep_chunk, sots_queue_stats *stats)
{
    // (what needs no handle is checked first, as above)
    if (stats) {
        if (stats->struct_size != sizeof(sots_queue_stats))
            return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_queue_stats.struct_size %u != %zu", stats->struct_size, sizeof(sots_queue_stats));
        stats->slots = 0;
        stats->global_generations = stats->chunk_generations = 0;
    }
    if (rule && stop_rule_check(rule))
        return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_batch_queue_run: stop rule with a wrong struct_size or check_interval 0");
    if (max_generations == 0) return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_batch_queue_run: max_generations must be at least 1");
    BATCH_REQUIRE(b);
    if (!b->track.best_ever()) return SOTS_FAIL(b, SOTS_ERR_STATE, "sots_batch_queue_run needs best-ever tracking: call sots_batch_track first");
    if (b->track.history())
        return SOTS_FAIL(b, SOTS_ERR_STATE, "sots_batch_queue_run keeps no per-slot history: call sots_batch_track without SOTS_TRACK_HISTORY");
    if (b->q_chunks == 0) return SOTS_FAIL(b, SOTS_ERR_STATE, "no queue: call sots_batch_queue_targets_audio or sots_batch_queue_targets_spectra first");
    // carry off: every chunk a segment of its own, and everything below is what it always was
    const QueuePlan plan = queue_plan(b->q_chunks, b->max_chunks, b->q_carry_rows, b->q_segment_chunks);
    const bool carry = b->q_carry_rows != 0;
    const uint32_t chunks = b->q_chunks, slots = plan.slots;
    if (keep_chunk != SOTS_QUEUE_NO_CHUNK && keep_chunk >= chunks)
        return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_batch_queue_run: keep_chunk %u not in 0..%u", keep_chunk, chunks - 1);
    // No chunk runs longer than max_generations, so the last one retires within `bound` loop generations (queue_loop_bound):
    // without a rule every slot turns over together and the loop below enqueues exactly that many.
    const uint64_t bound = queue_loop_bound(plan, max_generations, rule != nullptr);
    if (bound > 0xFFFFFFFFull) // (the loop generation is a 32-bit kernel argument)
        return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_batch_queue_run: %u chunks of up to %u generations in %u slots exceed 2^32 loop generations", chunks,
                     max_generations, slots);
    if (int rc = engine_bind(*b)) return rc;

    // the slots start with chunks 0..slots-1, exactly as sots_batch_set_target_spectra + sots_batch_init_population start them
    // (a carry run: slot c with chunk c * segment, the first of segment c; the head then counts segments)
    b->active = 0; // whatever happens from here on, the ordinary calls need their targets again
    b->q_ran = b->q_kept = false;
    std::vector<uint32_t> start(4 + 2 * (size_t)slots, 0u);
    start[0] = slots;
    for (uint32_t c = 0; c < slots; ++c) start[4 + 2 * c] = c * plan.segment;
    SOTS_HIP(b, hipMemcpyAsync(b->q_state, start.data(), start.size() * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
    if (!carry) {
        SOTS_HIP(b, launch_seg_targets(b->stream, b->seg_image, queue_targets(b), b->log2n, slots));
    } else { // one slot per launch: slot c's table from chunk c * segment's target (outside the loop: its cost does not matter)
        const size_t stride = seg_target_stride(b->log2n), half = b->N / 2;
        for (uint32_t c = 0; c < slots; ++c)
            SOTS_HIP(b, launch_seg_targets(b->stream, b->seg_image + (size_t)c * stride, queue_targets(b) + (size_t)c * plan.segment * half, b->log2n, 1));
    }
    SOTS_HIP(b, track_clear(b->track, b->stream));
    b->rot = 0;
    b->generation = 0;
    if (!carry) {
        SOTS_HIP(b, launch_init_population_seg(b->stream, b->val(0), b->stp(0), b->fit(0), b->pd, first_chunk_index, slots));
    } else {
        const size_t pop = (size_t)b->P * b->D;
        for (uint32_t c = 0; c < slots; ++c)
            SOTS_HIP(b, launch_init_population_seg(b->stream, b->val(0) + c * pop, b->stp(0) + c * pop, b->fit(0) + (size_t)c * b->P, b->pd,
                                                   first_chunk_index + c * plan.segment, 1));
    }
    SOTS_HIP(b, hipStreamSynchronize(b->stream)); // `start` leaves scope; the loop below starts from an empty stream

    QueueArgs q{};
    q.state = b->q_state;
    q.slot_table = b->q_state + 4;
    q.results = b->q_results;
    q.targets = queue_targets(b);
    q.seg_image = b->seg_image;
    q.kept_values = b->q_kept_rows;
    q.kept_steps = b->q_kept_rows + (size_t)b->P * b->D;
    q.kept_fitness = b->q_kept_rows + 2 * (size_t)b->P * b->D;
    q.num_chunks = chunks;
    q.first_chunk = first_chunk_index;
    q.max_generations = max_generations;
    q.keep_chunk = keep_chunk;
    q.check_interval = rule ? rule->check_interval : 0u;
    q.target_fitness = rule ? rule->target_fitness : -1.0f;
    q.stall_generations = rule ? rule->stall_generations : 0u;
    q.x_log2n = queue_x_log2n(b->log2n);
    q.half_bins = b->N / 2;
    q.carry_rows = b->q_carry_rows;
    q.segment_chunks = carry ? plan.segment : 0u;
    q.num_segments = carry ? plan.segments : 0u;

    // Blocks of check_interval generations; after each the queue's counters come back through a small asynchronous copy
    // to pinned memory.  The host waits for the copy of the block BEFORE the one it has just enqueued, so the device never
    // idles on the host; results are captured at retirement, so the block run past the end changes nothing.
    const uint32_t block = rule ? rule->check_interval : (max_generations < 32u ? max_generations : 32u);
    uint64_t global = 0, enqueued = 0, looked = 0; // generations and blocks enqueued, blocks whose counters the host has seen
    bool drained = false;
    uint32_t seen[4] = {0, 0, 0, 0};
    while (!drained) {
        if (global < bound) {
            for (uint32_t g = 0; g < block && global < bound; ++g) {
                if (int rc = enqueue_generation(b, slots, [b, &q, slots](uint32_t src, uint32_t dst) {
                        return launch_recombine_mutate_queue(b->stream, b->val(src), b->stp(src), b->val(dst), b->stp(dst), b->pd, b->mc,
                                                             q.slot_table, slots);
                    }))
                    return rc;
                global += 1;
                SOTS_HIP(b, launch_queue_turnover(b->stream, b->val(b->rot), b->stp(b->rot), b->fit(b->rot), b->pd, b->track.meta,
                                                   b->track.rows, q, (uint32_t)global, slots));
            }
            const uint32_t k = (uint32_t)(enqueued & 1u);
            SOTS_HIP(b, hipMemcpyAsync(b->q_pinned + 4 * k, b->q_state, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
            SOTS_HIP(b, hipEventRecord(b->q_event[k], b->stream));
            enqueued += 1;
            if (enqueued - looked < 2 && global < bound) continue; // stay one block ahead of the block looked at
        } else if (looked == enqueued) {
            return SOTS_FAIL(b, SOTS_ERR_STATE, "sots_batch_queue_run: %u of %u chunks retired after %llu generations", seen[1], chunks,
                         (unsigned long long)global);
        }
        const uint32_t k = (uint32_t)(looked & 1u);
        SOTS_HIP(b, hipEventSynchronize(b->q_event[k]));
        memcpy(seen, b->q_pinned + 4 * k, sizeof seen);
        looked += 1;
        drained = seen[1] >= chunks;
    }
    SOTS_HIP(b, hipStreamSynchronize(b->stream)); // the block enqueued ahead: nothing of it is kept
    b->generation = 0;
    b->q_ran = true;
    b->q_kept = keep_chunk != SOTS_QUEUE_NO_CHUNK;
    if (stats) {
        std::vector<uint32_t> run(chunks);
        SOTS_HIP(b, hipMemcpy2D(run.data(), sizeof(uint32_t), b->q_results, sizeof(sots_chunk_result), sizeof(uint32_t), chunks, hipMemcpyDeviceToHost));
        stats->slots = slots;
        stats->global_generations = seen[2];
        for (uint32_t r : run) stats->chunk_generations += r;
    }
    return SOTS_OK;
}

int sots_batch_queue_set_carry(sots_batch *b, uint32_t carry_rows, uint32_t segment_chunks)
{
    BATCH_REQUIRE(b);
    SOTS_REFUSE(b, queue_carry_check(carry_rows, segment_chunks, b->cfg.num_parents));
    b->q_carry_rows = carry_rows;
    b->q_segment_chunks = carry_rows ? segment_chunks : 0u;
    return SOTS_OK;
}

int sots_batch_queue_get_carry(const sots_batch *b, uint32_t *carry_rows, uint32_t *segment_chunks)
{
    BATCH_REQUIRE(b);
    if (!carry_rows || !segment_chunks) return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_batch_queue_get_carry: null pointer");
    *carry_rows = b->q_carry_rows;
    *segment_chunks = b->q_segment_chunks;
    return SOTS_OK;
}

int sots_batch_queue_results(sots_batch *b, sots_chunk_result *out, uint32_t capacity, uint32_t *written)
{
    BATCH_REQUIRE(b);
    if (written) *written = 0;
    if (!written || (capacity && !out)) return SOTS_FAIL(b, SOTS_ERR_INVALID, "sots_batch_queue_results: null argument");
    if (!b->q_ran) return SOTS_FAIL(b, SOTS_ERR_STATE, "no results: call sots_batch_queue_run first");
    if (int rc = engine_bind(*b)) return rc;
    const uint32_t n = capacity < b->q_chunks ? capacity : b->q_chunks;
    if (n) {
        SOTS_HIP(b, hipMemcpyAsync(out, b->q_results, (size_t)n * sizeof(sots_chunk_result), hipMemcpyDeviceToHost, b->stream));
        SOTS_HIP(b, hipStreamSynchronize(b->stream));
    }
    *written = n;
    return SOTS_OK;
}

int sots_batch_queue_read_kept_population(sots_batch *b, float *values, size_t values_bytes, float *steps, size_t steps_bytes,
                                          float *fitness, size_t fitness_bytes)
{
    BATCH_REQUIRE(b);
    if (!b->q_ran || !b->q_kept) return SOTS_FAIL(b, SOTS_ERR_STATE, "no kept population: call sots_batch_queue_run with a keep_chunk first");
    SOTS_REFUSE(b, population_bytes_check(b->P, b->D, values, values_bytes, steps, steps_bytes, fitness, fitness_bytes));
    if (int rc = engine_bind(*b)) return rc;
    const size_t pd_floats = (size_t)b->P * b->D;
    if (values) SOTS_HIP(b, hipMemcpyAsync(values, b->q_kept_rows, values_bytes, hipMemcpyDeviceToHost, b->stream));
    if (steps) SOTS_HIP(b, hipMemcpyAsync(steps, b->q_kept_rows + pd_floats, steps_bytes, hipMemcpyDeviceToHost, b->stream));
    if (fitness) SOTS_HIP(b, hipMemcpyAsync(fitness, b->q_kept_rows + 2 * pd_floats, fitness_bytes, hipMemcpyDeviceToHost, b->stream));
    SOTS_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

int sots_batch_read_best(sots_batch *b, float *values, size_t values_bytes, float *fitness, size_t fitness_bytes)
{
    BATCH_REQUIRE(b);
    if (int rc = require_active(b)) return rc;
    const size_t v_bytes = (size_t)b->active * b->D * sizeof(float), f_bytes = (size_t)b->active * sizeof(float);
    if ((values && values_bytes != v_bytes) || (fitness && fitness_bytes != f_bytes))
        return SOTS_FAIL(b, SOTS_ERR_SIZE, "best-row byte counts must be %zu (values) and %zu (fitness)", v_bytes, f_bytes);
    if (int rc = engine_bind(*b)) return rc;
    if (values)
        SOTS_HIP(b, hipMemcpy2DAsync(values, (size_t)b->D * sizeof(float), b->val(b->rot), (size_t)b->P * b->D * sizeof(float),
                                      (size_t)b->D * sizeof(float), b->active, hipMemcpyDeviceToHost, b->stream));
    if (fitness)
        SOTS_HIP(b, hipMemcpy2DAsync(fitness, sizeof(float), b->fit(b->rot), (size_t)b->P * sizeof(float), sizeof(float), b->active,
                                      hipMemcpyDeviceToHost, b->stream));
    SOTS_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

int sots_batch_read_population(sots_batch *b, uint32_t chunk, float *values, size_t values_bytes, float *steps, size_t steps_bytes,
                               float *fitness, size_t fitness_bytes)
{
    BATCH_REQUIRE(b);
    if (int rc = require_active(b)) return rc;
    if (chunk >= b->active) return SOTS_FAIL(b, SOTS_ERR_INVALID, "chunk %u not in 0..%u", chunk, b->active - 1);
    SOTS_REFUSE(b, population_bytes_check(b->P, b->D, values, values_bytes, steps, steps_bytes, fitness, fitness_bytes));
    if (int rc = engine_bind(*b)) return rc;
    const size_t row0 = (size_t)chunk * b->P;
    if (values) SOTS_HIP(b, hipMemcpyAsync(values, b->val(b->rot) + row0 * b->D, values_bytes, hipMemcpyDeviceToHost, b->stream));
    if (steps) SOTS_HIP(b, hipMemcpyAsync(steps, b->stp(b->rot) + row0 * b->D, steps_bytes, hipMemcpyDeviceToHost, b->stream));
    if (fitness) SOTS_HIP(b, hipMemcpyAsync(fitness, b->fit(b->rot) + row0, fitness_bytes, hipMemcpyDeviceToHost, b->stream));
    SOTS_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

} // extern "C"
