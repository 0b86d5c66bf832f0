// sots_engine.h -- what a context (sots_ctx, one population) and a batch (sots_batch, C chunk populations) have in
// common, in ONE copy that both handles embed: the configuration and what follows from it, the device and the stream,
// the host tables on the device, the objective, the synthesis launch and the error text.  Rows, rotation, selection and
// timing stay with the context; chunks, targets, the segmented image and the queue with the batch.  Host side only;
// internal to libsots_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sots_hip.h"
#include "sots_host_math.h"
#include "sots_kernels.h"
#include "sots_rules.h"

namespace sots {

// ---- failures: one routine, one HIP check ----
__attribute__((format(printf, 3, 4))) inline int fail_to(std::string &err, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}
// A file that uses the three macros below says where a handle's text goes: err_of(handle) is the handle's `err`, or for a
// null handle the file's own thread-local store (sots_last_error(NULL) and sots_batch_last_error(NULL) stay apart).
#define SOTS_FAIL(h, ...) sots::fail_to(err_of(h), __VA_ARGS__)
#define SOTS_REFUSE(h, fault_expr)                                               \
    do {                                                                         \
        if (const sots::Fault f_ = (fault_expr)) return SOTS_FAIL(h, f_.code, "%s", f_.text); \
    } while (0)
// on_fail runs with the code in rc_: `return rc_`, or a cleanup in front of it
#define SOTS_HIP_OR(h, call, on_fail)                                                                   \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess) {                                                                         \
            (void)hipGetLastError(); /* reported here: do not leave it for a later launch check */      \
            int rc_ = SOTS_FAIL(h, SOTS_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                                __FILE__, __LINE__);                                                    \
            on_fail;                                                                                    \
        }                                                                                               \
    } while (0)
#define SOTS_HIP(h, call) SOTS_HIP_OR(h, call, return rc_)

struct Engine {
    sots_config cfg{};
    sots_voice_graph graph{}; // SOTS_SYNTH_GRAPH: the topology that came with cfg (num_operators 0 for a fixed voice)
    uint32_t waveforms[8] = {0}; // ... and its operators' waveform codes (sots_set_voice_waveforms; all sine until set)
    float feedback[8] = {0};     // ... and their feedback indices (sots_set_voice_feedback; +0, no feedback, until set)
    uint32_t feedback_genes = 0; // ... and the operators whose index is a gene instead (sots_create_graph_genes; theirs above stays +0)
    uint32_t graph_form = SOTS_GRAPH_FORM_AUTO; // ... and the synthesis form asked for (sots_set_graph_synth_form): a preference, no state depends on it
    PopDims pd{};
    MutateConsts mc{};
    SynthParams sp{};
    int device = 0;
    uint32_t num_cus = 256;
    hipStream_t own_stream = nullptr, stream = nullptr; // stream: own_stream, or the caller's (sots_set_stream)
    uint32_t P = 0, D = 0, N = 0, log2n = 0;
    uint32_t pitch = 0; // floats between audio rows on the device (>= N)
    uint32_t synth_arith = SOTS_ARITH_CPU_PATH;
    float *wavetable = nullptr, *window = nullptr;
    float2 *twiddle = nullptr;
    float *x_image = nullptr; // k_fft_x's tables (N >= 2048): the context rebuilds them with every target, the batch makes them once
    OccCache occ{};
    // host tables
    std::vector<double> window64;
    float window_factor = 1.0f, inv_n = 0.0f, inv_wf = 1.0f;
    // the objective (sots_set_objective) and its per-bin weights (sots_set_objective_weights): u = sqrt(w) on the device
    // as plain bins and as the fused kernels read it; obj points at the two while weights are set
    Objective obj{};
    float *weights_u = nullptr, *weights_image = nullptr;
    mutable std::string err;
    char arch[32] = {0};
    char device_name[128] = {0};
};
inline std::string &err_of(const Engine &e) { return e.err; }

// The device, the stream, the sizes and constants of a configuration that config_check has passed, and the tables' device
// memory.  row_pad: floats behind the N of an audio row (rows off the power-of-two stride, see sots_kernels.h).  On a
// failure the text is in e.err and the caller releases.  graph: with SOTS_SYNTH_GRAPH, null otherwise; feedback_genes: its
// checked mask (sots_create_graph_genes), 0 from every other entry point.
inline int engine_create(Engine &e, const sots_config &cfg, const sots_voice_graph *graph, uint32_t row_pad, uint32_t feedback_genes = 0)
{
    int ndev = 0;
    hipError_t err = hipGetDeviceCount(&ndev);
    if (err != hipSuccess || ndev <= 0) return SOTS_FAIL(e, SOTS_ERR_NO_DEVICE, "no HIP device (%s)", hipGetErrorString(err));
    if (cfg.device < 0 || cfg.device >= ndev) return SOTS_FAIL(e, SOTS_ERR_NO_DEVICE, "device %d not in 0..%d", cfg.device, ndev - 1);
    e.cfg = cfg;
    if (graph) e.graph = *graph;
    e.feedback_genes = graph ? feedback_genes : 0u;
    e.device = cfg.device;
    SOTS_HIP(e, hipSetDevice(e.device));
    hipDeviceProp_t prop;
    SOTS_HIP(e, hipGetDeviceProperties(&prop, e.device));
    snprintf(e.arch, sizeof e.arch, "%s", prop.gcnArchName);
    snprintf(e.device_name, sizeof e.device_name, "%s", prop.name);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return SOTS_FAIL(e, SOTS_ERR_NO_DEVICE, "device %d is %s; libsots_hip carries gfx950 code only", e.device, prop.gcnArchName);
    e.num_cus = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256;
    SOTS_HIP(e, hipStreamCreateWithFlags(&e.own_stream, hipStreamNonBlocking));
    e.stream = e.own_stream;

    e.P = cfg.num_parents + cfg.num_offspring;
    e.D = graph ? graph_dims(graph->num_operators, e.feedback_genes) : dims_of(cfg.synth_kind);
    e.log2n = cfg.audio_length_log2;
    e.N = 1u << e.log2n;
    e.pitch = e.N + row_pad;
    e.pd = make_pop_dims(e.P, e.D, cfg.num_parents, cfg.workgroup_size, cfg.gid_base, (uint32_t)cfg.seed, (uint32_t)(cfg.seed >> 32));
    e.mc = mutate_consts(e.D);
    memcpy(e.sp.pmin, cfg.param_min, sizeof e.sp.pmin);
    memcpy(e.sp.pmax, cfg.param_max, sizeof e.sp.pmax);
    e.window64 = make_window(e.N, &e.window_factor);
    e.inv_n = 1.0f / (float)e.N;      // fftOneOverSize
    e.inv_wf = 1.f / e.window_factor; // fftOneOverWindowFactor

    SOTS_HIP(e, hipMalloc((void **)&e.wavetable, (size_t)SOTS_WAVETABLE_SIZE * sizeof(float)));
    SOTS_HIP(e, hipMalloc((void **)&e.window, (size_t)e.N * sizeof(float)));
    SOTS_HIP(e, hipMalloc((void **)&e.twiddle, (size_t)e.N * sizeof(float2)));
    if (e.log2n >= 11 && x_table_bytes(e.log2n)) SOTS_HIP(e, hipMalloc((void **)&e.x_image, x_table_bytes(e.log2n)));
    return SOTS_OK;
}

// host tables the reference also builds on the CPU and uploads (...OpenCL.hpp:315-317), enqueued behind whatever the handle
// has put on the stream for its own buffers.  `staging` is what the copies read: it lives until the caller has
// synchronised the stream.
struct TableStaging {
    std::vector<float> wavetable, window, twiddle;
};
inline int engine_upload_tables(Engine &e, TableStaging &staging)
{
    staging.wavetable = make_wavetable();
    staging.window.assign(e.window64.begin(), e.window64.end()); // (each double rounded to float)
    staging.twiddle = make_twiddles(e.N);
    SOTS_HIP(e, hipMemcpyAsync(e.wavetable, staging.wavetable.data(), staging.wavetable.size() * sizeof(float), hipMemcpyHostToDevice, e.stream));
    SOTS_HIP(e, hipMemcpyAsync(e.window, staging.window.data(), staging.window.size() * sizeof(float), hipMemcpyHostToDevice, e.stream));
    SOTS_HIP(e, hipMemcpyAsync(e.twiddle, staging.twiddle.data(), staging.twiddle.size() * sizeof(float), hipMemcpyHostToDevice, e.stream));
    return SOTS_OK;
}

// the caller has bound the device and synchronised the stream
inline void engine_release(Engine &e)
{
    void *bufs[] = {e.wavetable, e.window, e.twiddle, e.x_image, e.weights_u, e.weights_image};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (e.own_stream) (void)hipStreamDestroy(e.own_stream);
    (void)hipGetLastError(); // nothing sticky survives a handle (the launchers read hipGetLastError after each launch)
}

inline int engine_bind(const Engine &e)
{
    SOTS_HIP(e, hipSetDevice(e.device));
    return SOTS_OK;
}

// ---- settings ----
inline int engine_set_synth_arithmetic(Engine &e, uint32_t arith)
{
    SOTS_REFUSE(e, synth_arithmetic_check(arith, e.cfg.synth_kind));
    e.synth_arith = arith;
    return SOTS_OK;
}

inline int engine_set_survivors(Engine &e, uint32_t n)
{
    if (n > e.cfg.num_parents)
        return SOTS_FAIL(e, SOTS_ERR_INVALID, "%u survivors asked for, at most numParents = %u can be kept", n, e.cfg.num_parents);
    e.pd.survivors = n;
    return SOTS_OK;
}

// Checked before anything changes; the caller clears what a new voice makes stale (its run record, its stored splitters)
inline int engine_set_voice_waveforms(Engine &e, const uint32_t *codes, uint32_t count)
{
    SOTS_REFUSE(e, voice_waveforms_set(e.cfg.synth_kind, e.graph.num_operators, codes, count, e.waveforms));
    return SOTS_OK;
}
inline int engine_get_voice_waveforms(const Engine &e, uint32_t codes[8])
{
    if (!codes) return SOTS_FAIL(e, SOTS_ERR_INVALID, "voice waveforms: null argument");
    SOTS_REFUSE(e, voice_waveforms_check(e.cfg.synth_kind, e.graph.num_operators, nullptr, 0));
    memcpy(codes, e.waveforms, sizeof e.waveforms);
    return SOTS_OK;
}

inline int engine_set_voice_feedback(Engine &e, const float *index, uint32_t count)
{
    SOTS_REFUSE(e, voice_feedback_set(e.cfg.synth_kind, e.graph.num_operators, index, count, e.feedback, e.feedback_genes));
    return SOTS_OK;
}
inline int engine_get_voice_feedback(const Engine &e, float index[8])
{
    if (!index) return SOTS_FAIL(e, SOTS_ERR_INVALID, "voice feedback: null argument");
    SOTS_REFUSE(e, voice_feedback_check(e.cfg.synth_kind, e.graph.num_operators, nullptr, 0));
    memcpy(index, e.feedback, sizeof e.feedback);
    return SOTS_OK;
}

inline int engine_get_voice_feedback_genes(const Engine &e, uint32_t *feedback_genes)
{
    SOTS_REFUSE(e, voice_feedback_genes_get_check(e.cfg.synth_kind, feedback_genes));
    *feedback_genes = e.feedback_genes;
    return SOTS_OK;
}

// The synthesis form of the graph voice: a preference that changes no bit of any output, so nothing is cleared.
// own_rows: the rows of one synthesis of the handle's own population(s), for `effective`.
inline int engine_set_graph_synth_form(Engine &e, uint32_t form)
{
    SOTS_REFUSE(e, graph_synth_form_check(e.cfg.synth_kind, form));
    e.graph_form = form;
    return SOTS_OK;
}
inline int engine_get_graph_synth_form(const Engine &e, uint64_t own_rows, uint32_t *requested, uint32_t *effective)
{
    SOTS_REFUSE(e, graph_synth_form_check(e.cfg.synth_kind, SOTS_GRAPH_FORM_AUTO));
    if (!requested && !effective) return SOTS_FAIL(e, SOTS_ERR_INVALID, "graph synthesis form: null arguments");
    if (requested) *requested = e.graph_form;
    if (effective) *effective = graph_synth_form_for(e.graph_form, e.graph, e.feedback, e.feedback_genes, own_rows, e.num_cus);
    return SOTS_OK;
}

// ---- objective ----
// Both setters check everything before anything changes, then leave the objective they replaced in *old: the caller derives
// what depends on the new one (its target images, its run record) and, where that fails, puts *old back with
// engine_restore_objective.
inline int engine_set_objective(Engine &e, uint32_t objective, float floor, Objective *old)
{
    SOTS_REFUSE(e, objective_check(objective, floor));
    if (int rc = engine_bind(e)) return rc;
    *old = e.obj;
    e.obj.kind = objective;
    e.obj.floor = objective == SOTS_OBJECTIVE_LOG_MAGNITUDE ? floor : 0.0f;
    if (e.obj.kind != old->kind) occ_forget(e.occ); // (other kernels, other occupancies)
    return SOTS_OK;
}

// a table of N/2 weights and its length, or NULL and 0: no weights
inline int engine_set_objective_weights(Engine &e, const float *weights, uint32_t num_bins, Objective *old)
{
    std::vector<float> u;
    SOTS_REFUSE(e, objective_weights_fault(weights, num_bins, e.N / 2, u));
    if (int rc = engine_bind(e)) return rc;
    *old = e.obj;
    if (weights) {
        if (!e.weights_u) SOTS_HIP(e, hipMalloc((void **)&e.weights_u, (size_t)num_bins * sizeof(float)));
        if (!e.weights_image) SOTS_HIP(e, hipMalloc((void **)&e.weights_image, weight_image_bytes(e.log2n)));
        SOTS_HIP(e, hipMemcpyAsync(e.weights_u, u.data(), (size_t)num_bins * sizeof(float), hipMemcpyHostToDevice, e.stream));
        SOTS_HIP(e, launch_weight_image(e.stream, e.weights_image, e.weights_u, e.log2n));
        SOTS_HIP(e, hipStreamSynchronize(e.stream)); // (u goes out of scope)
        e.obj.weights = e.weights_u;
        e.obj.weights_image = e.weights_image;
    } else {
        e.obj.weights = e.obj.weights_image = nullptr;
    }
    if ((e.obj.weights != nullptr) != (old->weights != nullptr)) occ_forget(e.occ); // (other kernels, other occupancies)
    return SOTS_OK;
}

inline void engine_restore_objective(Engine &e, const Objective &old) { e.obj = old; }

// ---- synthesis ----
// audio[rows][pitch] from values[rows][D]: the arithmetic of the reference's device kernels where the handle asked for it
// (sots_set_synth_arithmetic; that compatibility kernel makes no individuals, the caller passes no Variation with it), the
// product's synthesis otherwise.  Raw audio: the window is applied by whoever reads the rows.
inline hipError_t engine_synthesise(const Engine &e, const float *values, float *audio, uint32_t rows, const Variation *var, bool allow_cut)
{
    if (e.synth_arith == SOTS_ARITH_DEVICE_KERNELS)
        return launch_synth_device_arith(e.stream, e.cfg.synth_kind, values, e.wavetable, audio, e.sp, rows, e.log2n, e.pitch);
    // the graph voice makes no individuals (launch_synth refuses a Variation with it): its launcher takes the handle's form
    if (e.cfg.synth_kind == SOTS_SYNTH_GRAPH && !var)
        return launch_synth_graph(e.stream, e.graph, values, e.wavetable, audio, e.sp, rows, e.log2n, e.pitch, e.num_cus, pack_waveforms(e.waveforms),
                                  e.feedback, e.feedback_genes, e.graph_form);
    return launch_synth(e.stream, e.cfg.synth_kind, values, e.wavetable, audio, e.sp, rows, e.log2n, e.pitch, e.num_cus, var, allow_cut, &e.graph,
                        pack_waveforms(e.waveforms), e.feedback, e.feedback_genes);
}

} // namespace sots
