// sots_batch.hip -- chunks in flight: the sots_batch_* entry points of include/sots_hip.h.  One handle advances C
// independent chunk populations, each against its own target, with the launches of ONE population per generation
// (variation | synthesis | window + FFT + fitness | sort, each over every chunk's rows).  Chunk c of a batch computes
// bit for bit what a sots_ctx of the same configuration computes for chunk first_chunk_index + c ("Chunks in
// flight").  No CPU fallback: every compute entry point launches gfx950 kernels or fails with an error code.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sots_hip.h"
#include "sots_host_math.h"
#include "sots_kernels.h"
#include "sots_stop_rule.h"
#include "sots_track.h"

using namespace sots;

namespace {
thread_local std::string g_batch_create_error;
constexpr uint32_t kBatchMaxPopulation = 1024; // one k_sort_small workgroup per chunk
constexpr uint64_t kQueueMaxTargetBytes = 1ull << 30; // the stored targets of a chunk queue (include/sots_hip.h)
static_assert(sizeof(sots_chunk_result) == 208 && sizeof(sots_chunk_result) == sots::kQueueResultFloats * sizeof(float),
              "sots_chunk_result is what k_queue_turnover writes");
} // namespace

struct sots_batch {
    sots_config cfg{};
    PopDims pd{};
    MutateConsts mc{};
    SynthParams sp{};
    int device = 0;
    uint32_t num_cus = 256;
    hipStream_t stream = nullptr;
    uint32_t P = 0, D = 0, N = 0, log2n = 0, pitch = 0;
    uint32_t max_chunks = 0, active = 0; // active: chunks of the last target call
    uint32_t rot = 0, generation = 0;
    uint32_t synth_arith = SOTS_ARITH_CPU_PATH;
    // device buffers; rows chunk-major, max_chunks * P per rotation half
    float *values = nullptr, *steps = nullptr, *fitness = nullptr; // [2][C P][D], [2][C P][D], [2][C P]
    float *audio = nullptr;                                        // [C P][pitch]
    float *targets = nullptr;                                      // [C][N/2] as uploaded
    // the objective of every chunk (sots_batch_set_objective).  Under LOG_MAGNITUDE the segmented image is laid out from
    // targets_ln = ln(targets + floor) and the queue's turnover reads q_targets_ln, both made on the device from the
    // uploaded magnitudes (batch_derive / queue_derive) and allocated with the first log objective that needs them
    Objective obj{};
    float *targets_ln = nullptr;                                   // [C][N/2]
    // per-bin weights of every chunk (sots_batch_set_objective_weights): one table, u = sqrt(w), as plain bins and as the
    // SEG kernels read it; b->obj points at the two while weights are set.  The targets' images do not depend on it.
    float *weights_u = nullptr, *weights_image = nullptr;
    float *seg_image = nullptr;                                    // segmented target image (sots_kernels.h)
    float *wavetable = nullptr, *window = nullptr, *x_image = nullptr;
    float2 *twiddle = nullptr;
    OccCache occ{};
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
    std::vector<double> window64;
    float window_factor = 1.0f, inv_n = 0.0f, inv_wf = 1.0f;
    mutable std::string err;

    size_t rows() const { return (size_t)max_chunks * P; }
    float *val(uint32_t half) const { return values + (size_t)half * rows() * D; }
    float *stp(uint32_t half) const { return steps + (size_t)half * rows() * D; }
    float *fit(uint32_t half) const { return fitness + (size_t)half * rows(); }
};

namespace {

int bfail(const sots_batch *b, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (b) b->err = buf;
    else g_batch_create_error = buf;
    return code;
}

#define BATCH_HIP(b, call)                                                                        \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (void)hipGetLastError();                                                              \
            return bfail(b, SOTS_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                         __FILE__, __LINE__);                                                     \
        }                                                                                         \
    } while (0)

#define BATCH_REQUIRE(b) \
    do {                 \
        if (!(b)) return bfail(nullptr, SOTS_ERR_INVALID, "null batch"); \
    } while (0)

uint32_t batch_dims_of(uint32_t kind)
{
    switch (kind) {
    case SOTS_SYNTH_2OP: return 4;
    case SOTS_SYNTH_3OP_SERIES: return 6;
    case SOTS_SYNTH_TRIPLE_PAR: return 12;
    case SOTS_SYNTH_4OP_SERIES: return 8;
    default: return 0;
    }
}

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
    void *bufs[] = {b->values, b->steps, b->fitness, b->audio, b->targets, b->targets_ln, b->weights_u, b->weights_image, b->seg_image,
                    b->wavetable, b->window, b->x_image, b->twiddle};
    for (void *p : bufs)
        if (p) (void)hipFree(p);
    track_release(b->track);
    queue_release(b);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    (void)hipGetLastError();
    delete b;
}

int bind(const sots_batch *b)
{
    BATCH_HIP(b, hipSetDevice(b->device));
    return SOTS_OK;
}

bool log_objective(const sots_batch *b) { return b->obj.kind == SOTS_OBJECTIVE_LOG_MAGNITUDE; }

// the segmented target image of chunks 0 .. num_chunks-1 from b->targets under b->obj; every chunk's record starts over
int batch_derive(sots_batch *b, uint32_t num_chunks)
{
    const float *src = b->targets;
    if (log_objective(b)) {
        const size_t m = b->N / 2;
        if (!b->targets_ln) BATCH_HIP(b, hipMalloc((void **)&b->targets_ln, (size_t)b->max_chunks * m * sizeof(float)));
        BATCH_HIP(b, launch_objective_map(b->stream, b->targets_ln, b->targets, (size_t)num_chunks * m, b->obj.floor));
        src = b->targets_ln;
    }
    BATCH_HIP(b, launch_seg_targets(b->stream, b->seg_image, src, b->log2n, num_chunks));
    BATCH_HIP(b, track_clear(b->track, b->stream));
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

// the stored queue targets as the turnover copies them into the image: the magnitudes, or their log image
int queue_derive(sots_batch *b)
{
    if (b->q_chunks == 0 || !log_objective(b)) return SOTS_OK;
    const size_t n = (size_t)b->q_chunks * (b->N / 2);
    if (!b->q_targets_ln) BATCH_HIP(b, hipMalloc((void **)&b->q_targets_ln, n * sizeof(float)));
    BATCH_HIP(b, launch_objective_map(b->stream, b->q_targets_ln, b->q_targets, n, b->obj.floor));
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}
const float *queue_targets(const sots_batch *b) { return log_objective(b) ? b->q_targets_ln : b->q_targets; }

int require_active(const sots_batch *b)
{
    if (b->active == 0)
        return bfail(b, SOTS_ERR_STATE, "no target: call sots_batch_set_target_audio or sots_batch_set_target_spectra first");
    return SOTS_OK;
}

} // namespace

extern "C" {

int sots_batch_create(const sots_config *cfg, uint32_t max_chunks, sots_batch **out)
{
    if (!cfg || !out) return bfail(nullptr, SOTS_ERR_INVALID, "sots_batch_create: null argument");
    *out = nullptr;
    // the configuration first, as sots_create: a machine without a GPU still tells a bad one from a good one
    if (cfg->struct_size != sizeof(sots_config))
        return bfail(nullptr, SOTS_ERR_INVALID, "sots_config.struct_size %u != %zu", cfg->struct_size, sizeof(sots_config));
    const uint32_t d = batch_dims_of(cfg->synth_kind);
    if (d == 0) return bfail(nullptr, SOTS_ERR_INVALID, "unknown synth_kind %u", cfg->synth_kind);
    if (cfg->num_dimensions != d)
        return bfail(nullptr, SOTS_ERR_INVALID, "synth_kind %u needs numDimensions %u, got %u", cfg->synth_kind, d, cfg->num_dimensions);
    if (cfg->audio_length_log2 < 8 || cfg->audio_length_log2 > 15)
        return bfail(nullptr, SOTS_ERR_INVALID, "audioLengthLog2 %u outside 8..15", cfg->audio_length_log2);
    const uint64_t p64 = (uint64_t)cfg->num_parents + cfg->num_offspring;
    if (cfg->num_parents == 0 || p64 < 2)
        return bfail(nullptr, SOTS_ERR_INVALID, "population %llu (parents %u) not supported", (unsigned long long)p64, cfg->num_parents);
    if (p64 > kBatchMaxPopulation)
        return bfail(nullptr, SOTS_ERR_INVALID, "a batch takes chunk populations of at most %u, got %llu (larger ones fill the GPU alone: sots_create)",
                     kBatchMaxPopulation, (unsigned long long)p64);
    if (cfg->workgroup_size == 0 || p64 % cfg->workgroup_size != 0)
        return bfail(nullptr, SOTS_ERR_INVALID, "populationLength %llu must be a multiple of workgroupSize %u (the recombination block)",
                     (unsigned long long)p64, cfg->workgroup_size);
    if (max_chunks == 0) return bfail(nullptr, SOTS_ERR_INVALID, "max_chunks must be at least 1");
    if ((uint64_t)max_chunks * p64 > (1ull << 26))
        return bfail(nullptr, SOTS_ERR_INVALID, "max_chunks %u x population %llu exceeds 2^26 rows", max_chunks, (unsigned long long)p64);

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return bfail(nullptr, SOTS_ERR_NO_DEVICE, "no HIP device (%s)", hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev)
        return bfail(nullptr, SOTS_ERR_NO_DEVICE, "device %d not in 0..%d", cfg->device, ndev - 1);

    sots_batch *b = new sots_batch();
    b->cfg = *cfg;
    b->device = cfg->device;
#define CREATE_HIP(call)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            int rc_ = bfail(nullptr, SOTS_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
            free_batch(b);                                                                        \
            return rc_;                                                                           \
        }                                                                                         \
    } while (0)
    CREATE_HIP(hipSetDevice(b->device));
    hipDeviceProp_t prop;
    CREATE_HIP(hipGetDeviceProperties(&prop, b->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        int rc = bfail(nullptr, SOTS_ERR_NO_DEVICE, "device %d is %s; libsots_hip carries gfx950 code only", b->device, prop.gcnArchName);
        free_batch(b);
        return rc;
    }
    b->num_cus = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256;
    CREATE_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));

    b->P = (uint32_t)p64;
    b->D = d;
    b->log2n = cfg->audio_length_log2;
    b->N = 1u << b->log2n;
    b->pitch = b->N + 32; // as sots_create: rows off the power-of-two stride
    b->max_chunks = max_chunks;
    b->pd = make_pop_dims(b->P, b->D, cfg->num_parents, cfg->workgroup_size, cfg->gid_base, (uint32_t)cfg->seed,
                          (uint32_t)(cfg->seed >> 32));
    // Evolutionary_Strategy.hpp:611-627, as sots_create
    const float mpi = (float)3.14159265358979323846;
    b->mc.alpha = 1.4f;
    b->mc.one_over_alpha = 1.f / b->mc.alpha;
    b->mc.root_two_over_pi = sqrtf(2.f / (float)mpi);
    b->mc.beta_scale = 1.f / (float)b->D;
    const float beta = sqrtf(b->mc.beta_scale);
    b->mc.pow_alpha_beta = powf(b->mc.alpha, beta);
    b->mc.pow_inv_alpha_beta = powf(b->mc.one_over_alpha, beta);
    memcpy(b->sp.pmin, cfg->param_min, sizeof b->sp.pmin);
    memcpy(b->sp.pmax, cfg->param_max, sizeof b->sp.pmax);

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
    CREATE_HIP(hipMalloc((void **)&b->wavetable, (size_t)SOTS_WAVETABLE_SIZE * sizeof(float)));
    CREATE_HIP(hipMalloc((void **)&b->window, (size_t)b->N * sizeof(float)));
    CREATE_HIP(hipMalloc((void **)&b->twiddle, (size_t)b->N * sizeof(float2)));
    if (b->log2n >= 11 && x_table_bytes(b->log2n)) CREATE_HIP(hipMalloc((void **)&b->x_image, x_table_bytes(b->log2n)));
    CREATE_HIP(hipMemsetAsync(b->values, 0, pd_bytes, b->stream));
    CREATE_HIP(hipMemsetAsync(b->steps, 0, pd_bytes, b->stream));
    CREATE_HIP(hipMemsetAsync(b->fitness, 0, (size_t)2 * b->rows() * sizeof(float), b->stream));
    CREATE_HIP(hipMemsetAsync(b->audio, 0, audio_bytes, b->stream));
    CREATE_HIP(hipMemsetAsync(b->targets, 0, targets_bytes, b->stream));
    CREATE_HIP(hipMemsetAsync(b->seg_image, 0, image_bytes, b->stream));

    const std::vector<float> table = make_wavetable();
    b->window64 = make_window(b->N, &b->window_factor);
    std::vector<float> window32(b->N);
    for (uint32_t i = 0; i < b->N; ++i) window32[i] = (float)b->window64[i];
    const std::vector<float> tw = make_twiddles(b->N);
    b->inv_n = 1.0f / (float)b->N;
    b->inv_wf = 1.f / b->window_factor;
    CREATE_HIP(hipMemcpyAsync(b->wavetable, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
    CREATE_HIP(hipMemcpyAsync(b->window, window32.data(), window32.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
    CREATE_HIP(hipMemcpyAsync(b->twiddle, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice, b->stream));
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

void sots_batch_destroy(sots_batch *b) { free_batch(b); }

const char *sots_batch_last_error(const sots_batch *b) { return b ? b->err.c_str() : g_batch_create_error.c_str(); }

int sots_batch_synchronize(sots_batch *b)
{
    BATCH_REQUIRE(b);
    if (int rc = bind(b)) return rc;
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

int sots_batch_set_target_spectra(sots_batch *b, const float *magnitudes, uint32_t num_bins, uint32_t num_chunks)
{
    BATCH_REQUIRE(b);
    if (num_chunks == 0 || num_chunks > b->max_chunks)
        return bfail(b, SOTS_ERR_INVALID, "num_chunks %u outside 1..%u", num_chunks, b->max_chunks);
    const uint64_t need = (uint64_t)num_chunks * (b->N / 2);
    if (!magnitudes || num_bins != need)
        return bfail(b, SOTS_ERR_SIZE, "%u target spectra need %llu bins, got %u", num_chunks, (unsigned long long)need, num_bins);
    if (int rc = bind(b)) return rc;
    BATCH_HIP(b, hipMemcpyAsync(b->targets, magnitudes, need * sizeof(float), hipMemcpyHostToDevice, b->stream));
    if (int rc = batch_derive(b, num_chunks)) return rc; // (new targets: every chunk's record starts over)
    b->active = num_chunks;
    return SOTS_OK;
}

int sots_batch_set_target_audio_hop(sots_batch *b, const float *audio, uint32_t num_samples, uint32_t hop, uint32_t num_chunks)
{
    BATCH_REQUIRE(b);
    if (num_chunks == 0 || num_chunks > b->max_chunks)
        return bfail(b, SOTS_ERR_INVALID, "num_chunks %u outside 1..%u", num_chunks, b->max_chunks);
    if (hop == 0 || hop > b->N) return bfail(b, SOTS_ERR_INVALID, "hop %u outside 1..%u", hop, b->N);
    const uint64_t need = (uint64_t)(num_chunks - 1u) * hop + b->N; // (hop = N: num_chunks * N)
    if (!audio || (uint64_t)num_samples < need)
        return bfail(b, SOTS_ERR_SIZE, "%u chunks of target audio need %llu samples, got %u", num_chunks, (unsigned long long)need, num_samples);
    const uint32_t m = b->N / 2;
    std::vector<float> mag((size_t)num_chunks * m);
    for (uint32_t c = 0; c < num_chunks; ++c) { // the single context's host transform, chunk by chunk
        const std::vector<float> one = target_spectrum(audio + (size_t)c * hop, b->N, b->window64, b->window_factor);
        memcpy(mag.data() + (size_t)c * m, one.data(), (size_t)m * sizeof(float));
    }
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
    if (int rc = bind(b)) return rc;
    b->rot = 0;
    b->generation = 0;
    BATCH_HIP(b, track_clear(b->track, b->stream));
    BATCH_HIP(b, launch_init_population_seg(b->stream, b->val(0), b->stp(0), b->fit(0), b->pd, first_chunk_index, b->active));
    return SOTS_OK;
}

int sots_batch_set_synth_arithmetic(sots_batch *b, uint32_t arith)
{
    BATCH_REQUIRE(b);
    if (arith > SOTS_ARITH_DEVICE_KERNELS) return bfail(b, SOTS_ERR_INVALID, "unknown synthesis arithmetic %u", arith);
    if (arith == SOTS_ARITH_DEVICE_KERNELS && b->cfg.synth_kind == SOTS_SYNTH_4OP_SERIES)
        return bfail(b, SOTS_ERR_INVALID, "the reference has no device kernel for the build-defined 4-op voice");
    b->synth_arith = arith;
    return SOTS_OK;
}

int sots_batch_set_survivors(sots_batch *b, uint32_t n)
{
    BATCH_REQUIRE(b);
    if (n > b->cfg.num_parents)
        return bfail(b, SOTS_ERR_INVALID, "%u survivors asked for, at most numParents = %u can be kept", n, b->cfg.num_parents);
    b->pd.survivors = n;
    return SOTS_OK;
}

int sots_batch_set_objective(sots_batch *b, uint32_t objective, float floor)
{
    BATCH_REQUIRE(b);
    if (objective != SOTS_OBJECTIVE_MAGNITUDE && objective != SOTS_OBJECTIVE_LOG_MAGNITUDE)
        return bfail(b, SOTS_ERR_INVALID, "unknown objective %u (0 = magnitude, 1 = log magnitude)", objective);
    if (objective == SOTS_OBJECTIVE_LOG_MAGNITUDE && !objective_floor_ok(floor))
        return bfail(b, SOTS_ERR_INVALID, "log-magnitude floor %g outside 1e-30 .. 1", (double)floor);
    if (int rc = bind(b)) return rc;
    const Objective old = b->obj;
    b->obj.kind = objective;
    b->obj.floor = objective == SOTS_OBJECTIVE_LOG_MAGNITUDE ? floor : 0.0f;
    if (b->obj.kind != old.kind) occ_forget(b->occ); // (other kernels, other occupancies)
    int rc = b->active ? batch_derive(b, b->active) : SOTS_OK;
    if (rc == SOTS_OK) rc = queue_derive(b);
    if (rc != SOTS_OK) b->obj = old, b->active = 0; // (the image may be half made: the ordinary calls need their targets again)
    return rc;
}

int sots_batch_set_objective_weights(sots_batch *b, const float *weights, uint32_t num_bins)
{
    BATCH_REQUIRE(b);
    if ((weights == nullptr) != (num_bins == 0))
        return bfail(b, SOTS_ERR_INVALID, "objective weights: a table and its length, or NULL and 0");
    std::vector<float> u;
    if (weights) {
        uint32_t bad = 0;
        switch (objective_weights_check(weights, num_bins, b->N / 2, u, &bad)) {
        case 1: return bfail(b, SOTS_ERR_INVALID, "objective weights need %u bins, got %u", b->N / 2, num_bins);
        case 2: return bfail(b, SOTS_ERR_INVALID, "objective weight %u is %g: every weight must be finite and >= 0", bad, (double)weights[bad]);
        case 3: return bfail(b, SOTS_ERR_INVALID, "objective weights are all zero");
        default: break;
        }
    }
    if (int rc = bind(b)) return rc;
    const Objective old = b->obj;
    if (weights) {
        if (!b->weights_u) BATCH_HIP(b, hipMalloc((void **)&b->weights_u, (size_t)num_bins * sizeof(float)));
        if (!b->weights_image) BATCH_HIP(b, hipMalloc((void **)&b->weights_image, weight_image_bytes(b->log2n)));
        BATCH_HIP(b, hipMemcpyAsync(b->weights_u, u.data(), (size_t)num_bins * sizeof(float), hipMemcpyHostToDevice, b->stream));
        BATCH_HIP(b, launch_weight_image(b->stream, b->weights_image, b->weights_u, b->log2n));
        BATCH_HIP(b, hipStreamSynchronize(b->stream)); // (u goes out of scope)
        b->obj.weights = b->weights_u;
        b->obj.weights_image = b->weights_image;
    } else {
        b->obj.weights = b->obj.weights_image = nullptr;
    }
    if ((b->obj.weights != nullptr) != (old.weights != nullptr)) occ_forget(b->occ); // (other kernels, other occupancies)
    // (the targets' images stay; what the chunks had found under the old weights says nothing: every record starts over)
    BATCH_HIP(b, track_clear(b->track, b->stream));
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

int sots_batch_execute_generations(sots_batch *b, uint32_t n)
{
    BATCH_REQUIRE(b);
    if (int rc = require_active(b)) return rc;
    if (int rc = bind(b)) return rc;
    const uint32_t rows = b->active * b->P;
    for (uint32_t g = 0; g < n; ++g) {
        // recombine + mutate, current half -> other half
        uint32_t src = b->rot, dst = b->rot ^ 1u;
        BATCH_HIP(b, launch_recombine_mutate_seg(b->stream, b->val(src), b->stp(src), b->val(dst), b->stp(dst), b->pd, b->mc,
                                                 b->generation, b->active));
        b->rot = dst;
        // synthesis: per row, so the single context's launcher serves every chunk's rows at once
        if (b->synth_arith == SOTS_ARITH_DEVICE_KERNELS)
            BATCH_HIP(b, launch_synth_device_arith(b->stream, b->cfg.synth_kind, b->val(b->rot), b->wavetable, b->audio, b->sp, rows,
                                                   b->log2n, b->pitch));
        else
            BATCH_HIP(b, launch_synth(b->stream, b->cfg.synth_kind, b->val(b->rot), b->wavetable, b->audio, b->sp, rows, b->log2n,
                                      b->pitch, b->num_cus, nullptr, true));
        // window + FFT + fitness, every row against its chunk's target
        BATCH_HIP(b, launch_fft_fitness_seg(b->stream, b->audio, b->window, b->seg_image, b->fit(b->rot), b->twiddle, rows, b->log2n,
                                            b->pitch, b->inv_n, b->inv_wf, b->num_cus, &b->occ, b->obj));
        // sortPopulation of every chunk (whole population: P <= 1024), current half -> other half
        src = b->rot, dst = b->rot ^ 1u;
        BATCH_HIP(b, launch_sort_seg(b->stream, b->val(src), b->stp(src), b->fit(src), b->val(dst), b->stp(dst), b->fit(dst), b->P,
                                     b->D, b->active));
        b->rot = dst;
        b->generation += 1;
        // the run record of every active chunk (nothing when tracking is off)
        BATCH_HIP(b, track_record(b->track, b->stream, b->val(b->rot), b->stp(b->rot), b->fit(b->rot), b->P, b->D, b->cfg.num_parents,
                                  b->generation, b->active));
    }
    return SOTS_OK;
}

// ---- run record: as sots_track and its readers, per chunk ----
int sots_batch_track(sots_batch *b, uint32_t flags, uint32_t history_every, uint32_t history_capacity)
{
    BATCH_REQUIRE(b);
    if (flags & ~(uint32_t)(SOTS_TRACK_BEST_EVER | SOTS_TRACK_HISTORY)) return bfail(b, SOTS_ERR_INVALID, "unknown track flags %u", flags);
    if (flags & SOTS_TRACK_HISTORY) {
        flags |= SOTS_TRACK_BEST_EVER;
        if (history_every == 0 || history_capacity == 0)
            return bfail(b, SOTS_ERR_INVALID, "history needs history_every >= 1 and history_capacity >= 1 (got %u, %u)", history_every, history_capacity);
        if ((uint64_t)history_capacity * b->max_chunks > kTrackMaxRecords)
            return bfail(b, SOTS_ERR_INVALID, "history_capacity %u x max_chunks %u exceeds %llu records", history_capacity, b->max_chunks,
                         (unsigned long long)kTrackMaxRecords);
    }
    if (int rc = bind(b)) return rc;
    BATCH_HIP(b, hipStreamSynchronize(b->stream)); // a record launch may still be using the old buffers
    BATCH_HIP(b, track_setup(b->track, flags, history_every, history_capacity, b->max_chunks, b->stream));
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

int sots_batch_read_best_ever(sots_batch *b, float *values, size_t values_bytes, float *steps, size_t steps_bytes, float *fitness,
                              size_t fitness_bytes, uint32_t *generation, size_t generation_bytes)
{
    BATCH_REQUIRE(b);
    if (int rc = require_active(b)) return rc;
    if (!b->track.best_ever()) return bfail(b, SOTS_ERR_STATE, "best-ever tracking is off: call sots_batch_track first");
    const size_t d_bytes = (size_t)b->D * sizeof(float), v_bytes = b->active * d_bytes, f_bytes = (size_t)b->active * sizeof(float);
    if ((values && values_bytes != v_bytes) || (steps && steps_bytes != v_bytes) || (fitness && fitness_bytes != f_bytes) ||
        (generation && generation_bytes != f_bytes))
        return bfail(b, SOTS_ERR_SIZE, "best-ever byte counts must be %zu (values, steps) and %zu (fitness, generation)", v_bytes, f_bytes);
    if (int rc = bind(b)) return rc;
    const size_t pitch = (size_t)kTrackRowFloats * sizeof(float);
    if (values)
        BATCH_HIP(b, hipMemcpy2DAsync(values, d_bytes, b->track.rows, pitch, d_bytes, b->active, hipMemcpyDeviceToHost, b->stream));
    if (steps)
        BATCH_HIP(b, hipMemcpy2DAsync(steps, d_bytes, b->track.rows + SOTS_MAX_DIMS, pitch, d_bytes, b->active, hipMemcpyDeviceToHost, b->stream));
    BATCH_HIP(b, track_fetch_meta(b->track, b->stream, b->active));
    for (uint32_t c = 0; c < b->active; ++c) {
        if (fitness) fitness[c] = track_fitness(b->track, c);
        if (generation) generation[c] = b->track.pinned[2 * c + 1];
    }
    return SOTS_OK;
}

int sots_batch_read_history(sots_batch *b, uint32_t chunk, sots_gen_record *out, uint32_t capacity, uint32_t *written, uint64_t *taken)
{
    BATCH_REQUIRE(b);
    if (!b->track.history()) return bfail(b, SOTS_ERR_STATE, "the history is off: call sots_batch_track with SOTS_TRACK_HISTORY first");
    if (int rc = require_active(b)) return rc;
    if (chunk >= b->active) return bfail(b, SOTS_ERR_INVALID, "chunk %u not in 0..%u", chunk, b->active - 1);
    if (!written || (capacity && !out)) return bfail(b, SOTS_ERR_INVALID, "read_history: null argument");
    if (int rc = bind(b)) return rc;
    BATCH_HIP(b, track_read_history(b->track, b->stream, chunk, out, capacity, written));
    if (taken) *taken = b->track.taken;
    return SOTS_OK;
}

int sots_batch_execute_until(sots_batch *b, uint32_t max_generations, const sots_stop_rule *rule, uint32_t *generations_run)
{
    BATCH_REQUIRE(b);
    if (generations_run) *generations_run = 0;
    if (sots_stop_rule_holds(rule, 0.0f, 0, 0) < 0) return bfail(b, SOTS_ERR_INVALID, "stop rule: null, wrong struct_size or check_interval 0");
    if (!b->track.best_ever()) return bfail(b, SOTS_ERR_STATE, "sots_batch_execute_until needs best-ever tracking: call sots_batch_track first");
    if (int rc = require_active(b)) return rc;
    uint32_t done = 0;
    while (done < max_generations) {
        const uint32_t block = rule->check_interval < max_generations - done ? rule->check_interval : max_generations - done;
        if (int rc = sots_batch_execute_generations(b, block)) return rc;
        done += block;
        if (generations_run) *generations_run = done;
        BATCH_HIP(b, track_fetch_meta(b->track, b->stream, b->active));
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
    if (num_chunks == 0) return bfail(b, SOTS_ERR_INVALID, "sots_batch_queue_targets: num_chunks must be at least 1");
    BATCH_REQUIRE(b);
    const uint64_t m = b->N / 2, need = (uint64_t)num_chunks * m;
    if (need * sizeof(float) > kQueueMaxTargetBytes)
        return bfail(b, SOTS_ERR_INVALID, "sots_batch_queue_targets: %u chunks of %llu bins exceed %llu bytes of stored targets", num_chunks,
                     (unsigned long long)m, (unsigned long long)kQueueMaxTargetBytes);
    if (!magnitudes || num_bins != need)
        return bfail(b, SOTS_ERR_SIZE, "%u queued target spectra need %llu bins, got %llu", num_chunks, (unsigned long long)need,
                     (unsigned long long)num_bins);
    if (int rc = bind(b)) return rc;
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    queue_release(b);
    const size_t pd_floats = (size_t)b->P * b->D;
#define QUEUE_HIP(call)                         \
    do {                                        \
        hipError_t e_ = (call);                 \
        if (e_ != hipSuccess) {                 \
            (void)hipGetLastError();            \
            queue_release(b);                   \
            return bfail(b, SOTS_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
        }                                       \
    } while (0)
    QUEUE_HIP(hipMalloc((void **)&b->q_targets, need * sizeof(float)));
    QUEUE_HIP(hipMalloc((void **)&b->q_results, (size_t)num_chunks * sizeof(sots_chunk_result)));
    QUEUE_HIP(hipMalloc((void **)&b->q_kept_rows, (2 * pd_floats + b->P) * sizeof(float)));
    QUEUE_HIP(hipMalloc((void **)&b->q_state, (4 + 2 * (size_t)b->max_chunks) * sizeof(uint32_t)));
    QUEUE_HIP(hipHostMalloc((void **)&b->q_pinned, 2 * 4 * sizeof(uint32_t), hipHostMallocDefault));
    for (hipEvent_t &e : b->q_event) QUEUE_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    QUEUE_HIP(hipMemcpyAsync(b->q_targets, magnitudes, need * sizeof(float), hipMemcpyHostToDevice, b->stream));
    QUEUE_HIP(hipStreamSynchronize(b->stream));
#undef QUEUE_HIP
    b->q_chunks = num_chunks;
    if (int rc = queue_derive(b)) {
        queue_release(b);
        return rc;
    }
    return SOTS_OK;
}

int sots_batch_queue_targets_audio_hop(sots_batch *b, const float *audio, uint64_t num_samples, uint32_t hop, uint32_t num_chunks)
{
    // (what needs no handle is checked first: a machine without a GPU still tells a bad call from a good one)
    if (num_chunks == 0) return bfail(b, SOTS_ERR_INVALID, "sots_batch_queue_targets: num_chunks must be at least 1");
    BATCH_REQUIRE(b);
    const uint64_t m = b->N / 2;
    if ((uint64_t)num_chunks * m * sizeof(float) > kQueueMaxTargetBytes)
        return bfail(b, SOTS_ERR_INVALID, "sots_batch_queue_targets: %u chunks of %llu bins exceed %llu bytes of stored targets", num_chunks,
                     (unsigned long long)m, (unsigned long long)kQueueMaxTargetBytes);
    if (hop == 0 || hop > b->N) return bfail(b, SOTS_ERR_INVALID, "sots_batch_queue_targets: hop %u outside 1..%u", hop, b->N);
    const uint64_t need = (uint64_t)(num_chunks - 1u) * hop + b->N; // (hop = N: num_chunks * N)
    if (!audio || num_samples < need)
        return bfail(b, SOTS_ERR_SIZE, "%u queued chunks of target audio need %llu samples, got %llu", num_chunks,
                     (unsigned long long)need, (unsigned long long)num_samples);
    std::vector<float> mag((size_t)num_chunks * m);
    for (uint32_t c = 0; c < num_chunks; ++c) { // the host transform of sots_batch_set_target_audio, chunk by chunk
        const std::vector<float> one = target_spectrum(audio + (size_t)c * hop, b->N, b->window64, b->window_factor);
        memcpy(mag.data() + (size_t)c * m, one.data(), (size_t)m * sizeof(float));
    }
    return sots_batch_queue_targets_spectra(b, mag.data(), mag.size(), num_chunks);
}

int sots_batch_queue_targets_audio(sots_batch *b, const float *audio, uint64_t num_samples, uint32_t num_chunks)
{
    // (what needs no handle is checked first: a machine without a GPU still tells a bad call from a good one)
    if (num_chunks == 0) return bfail(b, SOTS_ERR_INVALID, "sots_batch_queue_targets: num_chunks must be at least 1");
    BATCH_REQUIRE(b);
    return sots_batch_queue_targets_audio_hop(b, audio, num_samples, b->N, num_chunks);
}

int sots_batch_queue_run(sots_batch *b, uint32_t first_chunk_index, uint32_t max_generations, const sots_stop_rule *rule,
                         uint32_t keep_chunk, sots_queue_stats *stats)
{
    // (what needs no handle is checked first, as above)
    if (stats) {
        if (stats->struct_size != sizeof(sots_queue_stats))
            return bfail(b, SOTS_ERR_INVALID, "sots_queue_stats.struct_size %u != %zu", stats->struct_size, sizeof(sots_queue_stats));
        stats->slots = 0;
        stats->global_generations = stats->chunk_generations = 0;
    }
    if (rule && sots_stop_rule_holds(rule, 0.0f, 0, 0) < 0)
        return bfail(b, SOTS_ERR_INVALID, "sots_batch_queue_run: stop rule with a wrong struct_size or check_interval 0");
    if (max_generations == 0) return bfail(b, SOTS_ERR_INVALID, "sots_batch_queue_run: max_generations must be at least 1");
    BATCH_REQUIRE(b);
    if (!b->track.best_ever()) return bfail(b, SOTS_ERR_STATE, "sots_batch_queue_run needs best-ever tracking: call sots_batch_track first");
    if (b->track.history())
        return bfail(b, SOTS_ERR_STATE, "sots_batch_queue_run keeps no per-slot history: call sots_batch_track without SOTS_TRACK_HISTORY");
    if (b->q_chunks == 0) return bfail(b, SOTS_ERR_STATE, "no queue: call sots_batch_queue_targets_audio or sots_batch_queue_targets_spectra first");
    const uint32_t chunks = b->q_chunks, slots = chunks < b->max_chunks ? chunks : b->max_chunks;
    if (keep_chunk != SOTS_QUEUE_NO_CHUNK && keep_chunk >= chunks)
        return bfail(b, SOTS_ERR_INVALID, "sots_batch_queue_run: keep_chunk %u not in 0..%u", keep_chunk, chunks - 1);
    // No chunk runs longer than max_generations, so the last one retires within `bound` loop generations: without a rule
    // every slot turns over together and the loop below enqueues exactly that many.
    const uint64_t waves = ((uint64_t)chunks + slots - 1) / slots;
    const uint64_t bound = rule ? ((uint64_t)(chunks - 1) / slots + 2) * max_generations : waves * max_generations;
    if (bound > 0xFFFFFFFFull) // (the loop generation is a 32-bit kernel argument)
        return bfail(b, SOTS_ERR_INVALID, "sots_batch_queue_run: %u chunks of up to %u generations in %u slots exceed 2^32 loop generations", chunks,
                     max_generations, slots);
    if (int rc = bind(b)) return rc;

    // the slots start with chunks 0..slots-1, exactly as sots_batch_set_target_spectra + sots_batch_init_population start them
    b->active = 0; // whatever happens from here on, the ordinary calls need their targets again
    b->q_ran = b->q_kept = false;
    std::vector<uint32_t> start(4 + 2 * (size_t)slots, 0u);
    start[0] = slots;
    for (uint32_t c = 0; c < slots; ++c) start[4 + 2 * c] = c;
    BATCH_HIP(b, hipMemcpyAsync(b->q_state, start.data(), start.size() * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
    BATCH_HIP(b, launch_seg_targets(b->stream, b->seg_image, queue_targets(b), b->log2n, slots));
    BATCH_HIP(b, track_clear(b->track, b->stream));
    b->rot = 0;
    b->generation = 0;
    BATCH_HIP(b, launch_init_population_seg(b->stream, b->val(0), b->stp(0), b->fit(0), b->pd, first_chunk_index, slots));
    BATCH_HIP(b, hipStreamSynchronize(b->stream)); // `start` leaves scope; the loop below starts from an empty stream

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

    // Blocks of check_interval generations; after each the queue's counters come back through a small asynchronous copy
    // to pinned memory.  The host waits for the copy of the block BEFORE the one it has just enqueued, so the device never
    // idles on the host; results are captured at retirement, so the block run past the end changes nothing.
    const uint32_t block = rule ? rule->check_interval : (max_generations < 32u ? max_generations : 32u);
    const uint32_t rows = slots * b->P;
    uint64_t global = 0, enqueued = 0, looked = 0; // generations and blocks enqueued, blocks whose counters the host has seen
    bool drained = false;
    uint32_t seen[4] = {0, 0, 0, 0};
    while (!drained) {
        if (global < bound) {
            for (uint32_t g = 0; g < block && global < bound; ++g) {
                uint32_t src = b->rot, dst = b->rot ^ 1u;
                BATCH_HIP(b, launch_recombine_mutate_queue(b->stream, b->val(src), b->stp(src), b->val(dst), b->stp(dst), b->pd, b->mc,
                                                           q.slot_table, slots));
                b->rot = dst;
                if (b->synth_arith == SOTS_ARITH_DEVICE_KERNELS)
                    BATCH_HIP(b, launch_synth_device_arith(b->stream, b->cfg.synth_kind, b->val(b->rot), b->wavetable, b->audio, b->sp, rows,
                                                           b->log2n, b->pitch));
                else
                    BATCH_HIP(b, launch_synth(b->stream, b->cfg.synth_kind, b->val(b->rot), b->wavetable, b->audio, b->sp, rows, b->log2n,
                                              b->pitch, b->num_cus, nullptr, true));
                BATCH_HIP(b, launch_fft_fitness_seg(b->stream, b->audio, b->window, b->seg_image, b->fit(b->rot), b->twiddle, rows, b->log2n,
                                                    b->pitch, b->inv_n, b->inv_wf, b->num_cus, &b->occ, b->obj));
                src = b->rot, dst = b->rot ^ 1u;
                BATCH_HIP(b, launch_sort_seg(b->stream, b->val(src), b->stp(src), b->fit(src), b->val(dst), b->stp(dst), b->fit(dst), b->P,
                                             b->D, slots));
                b->rot = dst;
                global += 1;
                BATCH_HIP(b, launch_queue_turnover(b->stream, b->val(b->rot), b->stp(b->rot), b->fit(b->rot), b->pd, b->track.meta,
                                                   b->track.rows, q, (uint32_t)global, slots));
            }
            const uint32_t k = (uint32_t)(enqueued & 1u);
            BATCH_HIP(b, hipMemcpyAsync(b->q_pinned + 4 * k, b->q_state, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
            BATCH_HIP(b, hipEventRecord(b->q_event[k], b->stream));
            enqueued += 1;
            if (enqueued - looked < 2 && global < bound) continue; // stay one block ahead of the block looked at
        } else if (looked == enqueued) {
            return bfail(b, SOTS_ERR_STATE, "sots_batch_queue_run: %u of %u chunks retired after %llu generations", seen[1], chunks,
                         (unsigned long long)global);
        }
        const uint32_t k = (uint32_t)(looked & 1u);
        BATCH_HIP(b, hipEventSynchronize(b->q_event[k]));
        memcpy(seen, b->q_pinned + 4 * k, sizeof seen);
        looked += 1;
        drained = seen[1] >= chunks;
    }
    BATCH_HIP(b, hipStreamSynchronize(b->stream)); // the block enqueued ahead: nothing of it is kept
    b->generation = 0;
    b->q_ran = true;
    b->q_kept = keep_chunk != SOTS_QUEUE_NO_CHUNK;
    if (stats) {
        std::vector<uint32_t> run(chunks);
        BATCH_HIP(b, hipMemcpy2D(run.data(), sizeof(uint32_t), b->q_results, sizeof(sots_chunk_result), sizeof(uint32_t), chunks, hipMemcpyDeviceToHost));
        stats->slots = slots;
        stats->global_generations = seen[2];
        for (uint32_t r : run) stats->chunk_generations += r;
    }
    return SOTS_OK;
}

int sots_batch_queue_results(sots_batch *b, sots_chunk_result *out, uint32_t capacity, uint32_t *written)
{
    BATCH_REQUIRE(b);
    if (written) *written = 0;
    if (!written || (capacity && !out)) return bfail(b, SOTS_ERR_INVALID, "sots_batch_queue_results: null argument");
    if (!b->q_ran) return bfail(b, SOTS_ERR_STATE, "no results: call sots_batch_queue_run first");
    if (int rc = bind(b)) return rc;
    const uint32_t n = capacity < b->q_chunks ? capacity : b->q_chunks;
    if (n) {
        BATCH_HIP(b, hipMemcpyAsync(out, b->q_results, (size_t)n * sizeof(sots_chunk_result), hipMemcpyDeviceToHost, b->stream));
        BATCH_HIP(b, hipStreamSynchronize(b->stream));
    }
    *written = n;
    return SOTS_OK;
}

int sots_batch_queue_read_kept_population(sots_batch *b, float *values, size_t values_bytes, float *steps, size_t steps_bytes,
                                          float *fitness, size_t fitness_bytes)
{
    BATCH_REQUIRE(b);
    if (!b->q_ran || !b->q_kept) return bfail(b, SOTS_ERR_STATE, "no kept population: call sots_batch_queue_run with a keep_chunk first");
    const size_t pd_bytes = (size_t)b->P * b->D * sizeof(float), f_bytes = (size_t)b->P * sizeof(float);
    if ((values && values_bytes != pd_bytes) || (steps && steps_bytes != pd_bytes) || (fitness && fitness_bytes != f_bytes))
        return bfail(b, SOTS_ERR_SIZE, "population byte counts must be %zu (values, steps) and %zu (fitness)", pd_bytes, f_bytes);
    if (int rc = bind(b)) return rc;
    const size_t pd_floats = (size_t)b->P * b->D;
    if (values) BATCH_HIP(b, hipMemcpyAsync(values, b->q_kept_rows, pd_bytes, hipMemcpyDeviceToHost, b->stream));
    if (steps) BATCH_HIP(b, hipMemcpyAsync(steps, b->q_kept_rows + pd_floats, pd_bytes, hipMemcpyDeviceToHost, b->stream));
    if (fitness) BATCH_HIP(b, hipMemcpyAsync(fitness, b->q_kept_rows + 2 * pd_floats, f_bytes, hipMemcpyDeviceToHost, b->stream));
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

int sots_batch_read_best(sots_batch *b, float *values, size_t values_bytes, float *fitness, size_t fitness_bytes)
{
    BATCH_REQUIRE(b);
    if (int rc = require_active(b)) return rc;
    const size_t v_bytes = (size_t)b->active * b->D * sizeof(float), f_bytes = (size_t)b->active * sizeof(float);
    if ((values && values_bytes != v_bytes) || (fitness && fitness_bytes != f_bytes))
        return bfail(b, SOTS_ERR_SIZE, "best-row byte counts must be %zu (values) and %zu (fitness)", v_bytes, f_bytes);
    if (int rc = bind(b)) return rc;
    if (values)
        BATCH_HIP(b, hipMemcpy2DAsync(values, (size_t)b->D * sizeof(float), b->val(b->rot), (size_t)b->P * b->D * sizeof(float),
                                      (size_t)b->D * sizeof(float), b->active, hipMemcpyDeviceToHost, b->stream));
    if (fitness)
        BATCH_HIP(b, hipMemcpy2DAsync(fitness, sizeof(float), b->fit(b->rot), (size_t)b->P * sizeof(float), sizeof(float), b->active,
                                      hipMemcpyDeviceToHost, b->stream));
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

int sots_batch_read_population(sots_batch *b, uint32_t chunk, float *values, size_t values_bytes, float *steps, size_t steps_bytes,
                               float *fitness, size_t fitness_bytes)
{
    BATCH_REQUIRE(b);
    if (int rc = require_active(b)) return rc;
    if (chunk >= b->active) return bfail(b, SOTS_ERR_INVALID, "chunk %u not in 0..%u", chunk, b->active - 1);
    const size_t pd_bytes = (size_t)b->P * b->D * sizeof(float), f_bytes = (size_t)b->P * sizeof(float);
    if ((values && values_bytes != pd_bytes) || (steps && steps_bytes != pd_bytes) || (fitness && fitness_bytes != f_bytes))
        return bfail(b, SOTS_ERR_SIZE, "population byte counts must be %zu (values, steps) and %zu (fitness)", pd_bytes, f_bytes);
    if (int rc = bind(b)) return rc;
    const size_t row0 = (size_t)chunk * b->P;
    if (values) BATCH_HIP(b, hipMemcpyAsync(values, b->val(b->rot) + row0 * b->D, pd_bytes, hipMemcpyDeviceToHost, b->stream));
    if (steps) BATCH_HIP(b, hipMemcpyAsync(steps, b->stp(b->rot) + row0 * b->D, pd_bytes, hipMemcpyDeviceToHost, b->stream));
    if (fitness) BATCH_HIP(b, hipMemcpyAsync(fitness, b->fit(b->rot) + row0, f_bytes, hipMemcpyDeviceToHost, b->stream));
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    return SOTS_OK;
}

} // extern "C"
