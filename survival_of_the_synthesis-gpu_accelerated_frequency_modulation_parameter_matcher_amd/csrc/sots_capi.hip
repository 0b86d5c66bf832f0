// sots_capi.hip -- the C-ABI of include/sots_hip.h: context, buffers, stage sequencing,
// device timing.  No CPU fallback exists: every compute entry point launches gfx950 kernels
// or fails with an error code.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sots_hip.h"
#include "sots_engine.h"
#include "sots_host_math.h"
#include "sots_kernels.h"
#include "sots_render.h"
#include "sots_stop_rule.h"
#include "sots_track.h"

using namespace sots;

namespace {

struct StageClock {
    // recorded, not yet read.  Inside the fused generation loop consecutive stages SHARE the event between them (the
    // end of one is the start of the next: one event record per kernel boundary instead of two), so an event may
    // sit in two pairs; events are owned by the context's pool and go back to it once every clock has been read.
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double total_ms = 0.0;
    uint64_t count = 0;
    std::vector<float> launches_ms; // per-launch durations since the last reset (bounded: kMaxLaunchSamples)
};
constexpr size_t kMaxLaunchSamples = 1u << 16;

thread_local std::string g_create_error;

} // namespace

struct sots_ctx : sots::Engine {
    uint32_t rot = 0, generation = 0;
    bool target_set = false;
    // device buffers
    float *values = nullptr, *steps = nullptr, *fitness = nullptr; // [2][P][D], [2][P][D], [2][P]
    float *audio = nullptr, *spectrum = nullptr, *target = nullptr, *rows = nullptr;
    uint64_t *keys = nullptr;
    void *sort_scratch = nullptr;
    uint32_t rows_capacity = 0;
    // Under SOTS_OBJECTIVE_LOG_MAGNITUDE the spectral kernels read target_ln = ln(target + floor), made on the device from
    // `target` (which stays the raw magnitudes) whenever the target or the objective changes; allocated with the first
    // log objective
    float *target_ln = nullptr;
    std::vector<float> weights_w; // the per-bin weights as passed (sots_get_objective_weights)
    // selection state: after the fused loop's partial sort only rows [0, tail_first) of the current half
    // are in place; the unsorted half it came from is intact until the next generation starts
    uint32_t sort_mode = SOTS_SORT_LAZY_TAIL;
    bool tail_pending = false;
    uint32_t tail_first = 0;
    // the one-launch selection (k_sel_splitters): two slots of splitters, read and written in turn.  spl_valid: the
    // slot spl_cur was written by the last selection of THIS population (a promise of speed only: any slot content
    // gives the exact rows)
    uint64_t *splitters = nullptr;
    uint32_t spl_cur = 0;
    bool spl_valid = false;
    // list mode of that selection: the spectral kernel files every key under its bucket between the
    // splitters of slot spl_cur - counter set spl_cur, the key lists - and the selection reads its bucket from there.
    // A set must be all zero when a launch starts to count into it: the selection that consumes set s clears set s ^ 1
    // for the next generation, and cnt_dirty (bit s: set s may hold counts) makes the host clear a set that a generation
    // without lists, an invalidation or a failed call has left behind.  lists_ready: sots_stage_bucket_fitness has
    // filed the current half's fitness for the next sots_stage_select.
    uint32_t *sel_cnt = nullptr;
    uint64_t *sel_lists = nullptr;
    uint32_t cnt_dirty = 0;
    bool use_lists = true, lists_ready = false;
    uint32_t select_plan = SOTS_SELECT_AUTO;
    // island exchange folded into the sort of the last generation of the next sots_execute_generations call
    // run record (sots_track): best-ever individual and history, updated by one launch after each generation's sort
    TrackState track{};
    SortExchange next_exchange{};
    bool next_exchange_set = false;
    hipEvent_t next_exchange_gate = nullptr; // the HOST waits for it right before that sort is enqueued
    // overlap-add rendering (sots_render_overlap_add): scratch of its own, allocated by the first rendering
    RenderScratch render{};
    // experiment switches; fixed in the shipped library, settable from the environment only in a
    // -DSOTS_EXPERIMENT build (tools/exp_*.sh)
    bool allow_cut = true;
    int skip_stage = 0;
    int fuse_variation = -1; // -1: by population shape, 0 / 1: forced
    // timing
    bool timing = false;
    std::vector<hipEvent_t> event_pool;
    hipEvent_t chain_tail = nullptr; // fused loop: the event the last stage ended with
    StageClock clocks[SOTS_STAGE_COUNT];

    float *val(uint32_t half) const { return values + (size_t)half * P * D; }
    float *stp(uint32_t half) const { return steps + (size_t)half * P * D; }
    float *fit(uint32_t half) const { return fitness + (size_t)half * P; }
};

namespace {

std::string &err_of(const sots_ctx *ctx) { return ctx ? ctx->err : g_create_error; }

#define SOTS_REQUIRE_CTX(ctx) \
    do {                      \
        if (!(ctx)) return SOTS_FAIL(nullptr, SOTS_ERR_INVALID, "null context"); \
    } while (0)

// ---- stage timing -------------------------------------------------------------------
hipEvent_t take_event(sots_ctx *c)
{
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// CHAIN (the fused generation loop, where the stages follow each other on the stream with nothing in between): the
// stage starts at the event the stage before it ended with.
struct StageScope {
    sots_ctx *ctx;
    StageClock *clock = nullptr;
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    bool chain;
    StageScope(sots_ctx *c, int stage, bool chained = false) : ctx(c), chain(chained)
    {
        if (!c->timing) return;
        if (chain && c->chain_tail) {
            ev.first = c->chain_tail;
        } else {
            ev.first = take_event(c);
            if (ev.first) (void)hipEventRecord(ev.first, c->stream);
        }
        ev.second = take_event(c);
        if (!ev.first || !ev.second) { // (a lost pair costs a sample, nothing else)
            if (ev.first && ev.first != c->chain_tail) c->event_pool.push_back(ev.first);
            if (ev.second) c->event_pool.push_back(ev.second);
            return;
        }
        clock = &c->clocks[stage];
    }
    ~StageScope()
    {
        if (!clock) return;
        (void)hipEventRecord(ev.second, ctx->stream);
        clock->pending.push_back(ev);
        if (chain) ctx->chain_tail = ev.second;
    }
};

// reads every recorded pair of every stage and returns the events to the pool
int drain_clocks(sots_ctx *ctx)
{
    std::vector<hipEvent_t> used;
    int rc = SOTS_OK;
    for (auto &ck : ctx->clocks) {
        for (auto &ev : ck.pending) {
            used.push_back(ev.first);
            used.push_back(ev.second);
            if (rc) continue;
            float ms = 0.0f;
            if (hipEventSynchronize(ev.second) != hipSuccess || hipEventElapsedTime(&ms, ev.first, ev.second) != hipSuccess) {
                rc = SOTS_FAIL(ctx, SOTS_ERR_HIP, "stage timing: %s", hipGetErrorString(hipGetLastError()));
                continue;
            }
            ck.total_ms += ms;
            ck.count += 1;
            if (ck.launches_ms.size() < kMaxLaunchSamples) ck.launches_ms.push_back(ms);
        }
        ck.pending.clear();
    }
    std::sort(used.begin(), used.end());
    used.erase(std::unique(used.begin(), used.end()), used.end());
    ctx->event_pool.insert(ctx->event_pool.end(), used.begin(), used.end());
    ctx->chain_tail = nullptr;
    return rc;
}

// keep the number of live events bounded on long runs
int maybe_drain(sots_ctx *ctx)
{
    if (!ctx->timing) return SOTS_OK;
    for (auto &ck : ctx->clocks)
        if (ck.pending.size() >= 4096) return drain_clocks(ctx);
    return SOTS_OK;
}

void free_ctx(sots_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    {
        std::vector<hipEvent_t> all = ctx->event_pool;
        for (auto &ck : ctx->clocks)
            for (auto &ev : ck.pending) all.push_back(ev.first), all.push_back(ev.second);
        std::sort(all.begin(), all.end());
        all.erase(std::unique(all.begin(), all.end()), all.end());
        for (hipEvent_t e : all) (void)hipEventDestroy(e);
    }
    void *bufs[] = {ctx->values, ctx->steps, ctx->fitness, ctx->audio, ctx->spectrum, ctx->target, ctx->target_ln, ctx->rows, ctx->keys,
                    ctx->sort_scratch, ctx->splitters, ctx->sel_cnt, ctx->sel_lists};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    track_release(ctx->track);
    render_release(ctx->render);
    engine_release(*ctx);
    delete ctx;
}

// a creation that fails: its text outlives the handle in the thread's store
int abandon(sots_ctx *ctx, int rc)
{
    g_create_error = ctx->err;
    free_ctx(ctx);
    return rc;
}

int ensure_rows(sots_ctx *ctx, uint32_t n_rows)
{
    if (n_rows <= ctx->rows_capacity) return SOTS_OK;
    if (ctx->rows) SOTS_HIP(ctx, hipFree(ctx->rows));
    ctx->rows = nullptr;
    ctx->rows_capacity = 0;
    SOTS_HIP(ctx, hipMalloc((void **)&ctx->rows, (size_t)n_rows * (2 * ctx->D + 1) * sizeof(float)));
    ctx->rows_capacity = n_rows;
    return SOTS_OK;
}

// the rows recombination reads and the rows the selection places (sots_rules.h), of this context
uint32_t breeding_rows(const sots_ctx *ctx) { return sots::breeding_rows(ctx->cfg.num_parents, ctx->pd.block); }
uint32_t selected_rows(const sots_ctx *ctx) { return sots::selected_rows(ctx->cfg.num_parents, ctx->pd.block); }

// Produces the rows the selection left out: the full sort of the (still intact) unsorted half, writing
// only rows >= tail_first of the current half (the rows in front are in place, immigrants included).
int complete_tail(sots_ctx *ctx)
{
    if (!ctx->tail_pending) return SOTS_OK;
    if (ctx->sort_mode == SOTS_SORT_TOP_ONLY) return SOTS_OK; // the caller asked for the selected rows only
    SOTS_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t dst = ctx->rot, src = ctx->rot ^ 1u, first = ctx->tail_first;
    if (first == 0) { // sots_stage_select without its sots_stage_rotate yet: the selected rows are in the other half
        dst = ctx->rot ^ 1u;
        src = ctx->rot;
        first = selected_rows(ctx);
    }
    {
        StageScope t(ctx, SOTS_STAGE_SORT_TAIL);
        SOTS_HIP(ctx, launch_sort(ctx->stream, ctx->val(src), ctx->stp(src), ctx->fit(src), ctx->val(dst), ctx->stp(dst),
                                  ctx->fit(dst), ctx->keys, ctx->sort_scratch, ctx->P, ctx->D, first));
    }
    ctx->tail_pending = false;
    return SOTS_OK;
}

// For every call that is about to WRITE population rows (a stage, write_population): the rows the selection left
// out are produced first (SOTS_SORT_LAZY_TAIL), and whatever the mode the pending state ends here - the half it would
// be completed from, or the rows it would fill, are about to change.  In SOTS_SORT_TOP_ONLY nothing is produced
// (rows >= S stay unspecified); pure reads keep the state in that mode, so switching to SOTS_SORT_LAZY_TAIL while the
// unsorted half is still intact completes it.
int settle_tail(sots_ctx *ctx)
{
    if (int rc = complete_tail(ctx)) return rc;
    ctx->tail_pending = false;
    ctx->tail_first = 0;
    ctx->spl_valid = false; // rows or fitness are about to change under the stored splitters
    ctx->lists_ready = false;
    return SOTS_OK;
}

uint64_t *splitter_slot(const sots_ctx *ctx, uint32_t which)
{
    return ctx->splitters + (size_t)which * (select_splitter_slot_bytes() / sizeof(uint64_t));
}

// list mode: can keys be filed between this context's splitters at all (a slot that fits the filing kernels' LDS)?
bool lists_possible(const sots_ctx *ctx)
{
    return ctx->use_lists && ctx->sel_cnt && ctx->sel_lists && select_splitter_count(ctx->num_cus) <= kSelListMaxBuckets;
}

// ... and does the fused loop's spectral kernel file them (the wide N = 1024 kernel)?
bool lists_in_loop(const sots_ctx *ctx)
{
    return lists_possible(ctx) && ctx->skip_stage == 0 && select_lists_apply(ctx->P, ctx->log2n, ctx->num_cus);
}

// does sortPopulation of the fused loop (or sots_stage_select) take the one-launch selection now?  SPLITTERS: always;
// AUTO: when the slot holds the last selection's splitters and P <= 65536 - or P <= 131072, the largest population the
// two-launch selection handles, where the loop runs in list mode: the streaming kernel's cost grows with P x B and has
// not been compared with the two launches there, list mode's does not, and at 131072 it won every round of the A/B
// (profiles/r08_experiments.md)
#ifndef SOTS_AUTO_MAX_P
#define SOTS_AUTO_MAX_P 131072u // (65536u: the build variant of the A/B at 131072, profiles/r08_experiments.md)
#endif
bool use_splitters(const sots_ctx *ctx)
{
    if (ctx->select_plan == SOTS_SELECT_SPLITTERS) return true;
    if (ctx->select_plan == SOTS_SELECT_TILES) return false;
    return ctx->spl_valid && (ctx->P <= 65536u || (ctx->P <= SOTS_AUTO_MAX_P && lists_in_loop(ctx)));
}

uint32_t *counter_set(const sots_ctx *ctx, uint32_t which) { return ctx->sel_cnt + (size_t)which * (select_counters_bytes() / sizeof(uint32_t)); }

SelLists lists_of(const sots_ctx *ctx)
{
    return SelLists{splitter_slot(ctx, ctx->spl_cur), counter_set(ctx, ctx->spl_cur), counter_set(ctx, ctx->spl_cur ^ 1u), ctx->sel_lists,
                    select_splitter_count(ctx->num_cus)};
}

// in front of a launch that files keys between the splitters of slot spl_cur: its counter set is all zero
int open_lists(sots_ctx *ctx, SelLists *out)
{
    const uint32_t bit = 1u << ctx->spl_cur;
    if (ctx->cnt_dirty & bit) SOTS_HIP(ctx, hipMemsetAsync(counter_set(ctx, ctx->spl_cur), 0, select_counters_bytes(), ctx->stream));
    ctx->cnt_dirty |= bit;
    *out = lists_of(ctx);
    return SOTS_OK;
}

// the selection of rows 0..need-1 from half src into half dst, by the plan in force.  lists: the keys of half src have
// been filed between the splitters of slot spl_cur (open_lists) - the one-launch selection only
int run_select(sots_ctx *ctx, uint32_t src, uint32_t dst, uint32_t need, const SortExchange *ex, bool lists = false)
{
    if (use_splitters(ctx)) {
        const SelLists sl = lists_of(ctx);
        SOTS_HIP(ctx, launch_select_splitters(ctx->stream, ctx->val(src), ctx->stp(src), ctx->fit(src), ctx->val(dst), ctx->stp(dst),
                                              ctx->fit(dst), ctx->keys, splitter_slot(ctx, ctx->spl_cur), splitter_slot(ctx, ctx->spl_cur ^ 1u),
                                              ctx->P, ctx->D, need, ctx->num_cus, ex, lists ? &sl : nullptr));
        if (lists) ctx->cnt_dirty &= ~(1u << (ctx->spl_cur ^ 1u)); // cleared by that launch: the next generation counts into it
    } else {
        SOTS_HIP(ctx, launch_select(ctx->stream, ctx->val(src), ctx->stp(src), ctx->fit(src), ctx->val(dst), ctx->stp(dst),
                                    ctx->fit(dst), ctx->keys, ctx->sort_scratch, ctx->P, ctx->D, need, ctx->num_cus, ex));
        if (ctx->select_plan == SOTS_SELECT_TILES || (ctx->P > 65536u && !(ctx->P <= SOTS_AUTO_MAX_P && lists_in_loop(ctx)))) return SOTS_OK; // nobody will read a slot
        // the sorted fitness just written seeds the other slot for the next generation
        SOTS_HIP(ctx, launch_select_seed(ctx->stream, ctx->fit(dst), splitter_slot(ctx, ctx->spl_cur ^ 1u), need, ctx->num_cus));
    }
    ctx->spl_cur ^= 1u;
    ctx->spl_valid = true;
    return SOTS_OK;
}

// the bins the fitness kernels read: the magnitudes, or their image under the log objective
const float *fitness_target(const sots_ctx *ctx)
{
    return ctx->obj.kind == SOTS_OBJECTIVE_LOG_MAGNITUDE ? ctx->target_ln : ctx->target;
}

// What follows from ctx->target and ctx->obj: the log image, the long rows' tables in the layout the fused kernel reads
// them in.  Also what a new target or objective makes stale: the run record, the stored splitters, the key lists.
int derive_target(sots_ctx *ctx)
{
    if (ctx->obj.kind == SOTS_OBJECTIVE_LOG_MAGNITUDE) {
        if (!ctx->target_ln) SOTS_HIP(ctx, hipMalloc((void **)&ctx->target_ln, (size_t)(ctx->N / 2) * sizeof(float)));
        SOTS_HIP(ctx, launch_objective_map(ctx->stream, ctx->target_ln, ctx->target, ctx->N / 2, ctx->obj.floor));
    }
    if (ctx->x_image) { // long rows: the fused spectral kernel's tables, in the layout it reads them in
        SOTS_HIP(ctx, launch_x_tables(ctx->stream, ctx->x_image, ctx->twiddle, ctx->window, fitness_target(ctx), ctx->log2n));
        ctx->occ.x_image = ctx->x_image;
    }
    SOTS_HIP(ctx, track_clear(ctx->track, ctx->stream)); // a new target: what was best against the old one says nothing
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->spl_valid = false; // the fitness landscape changes
    ctx->lists_ready = false;
    return SOTS_OK;
}

int require_target(sots_ctx *ctx)
{
    if (!ctx->target_set)
        return SOTS_FAIL(ctx, SOTS_ERR_STATE, "no target: call sots_set_target_audio or sots_set_target_spectrum first");
    return SOTS_OK;
}

// the run record of the generation whose sort has just been enqueued: the current half, the counter after it
int record_generation(sots_ctx *ctx)
{
    if (!ctx->track.flags) return SOTS_OK;
    SOTS_HIP(ctx, track_record(ctx->track, ctx->stream, ctx->val(ctx->rot), ctx->stp(ctx->rot), ctx->fit(ctx->rot), ctx->P, ctx->D,
                               ctx->cfg.num_parents, ctx->generation, 1));
    return SOTS_OK;
}

// ---- phase-continuous rendering: the passes ----
// What the three entry points share once their checks have passed: the passes.  `who` names the entry point in a refusal;
// cap: the most samples its scratch lets a pass hold; layout(samples): its pass struct (ContPass, GraphPass) for passes of so
// many samples, with .lay and whatever else is its own filled in; state_words: the words from lay.carry on that a pass
// leaves for the next, cleared before the first; launch(pass, rows) enqueues one pass, whose `rows` rows from pass.row_base on
// are on the device.  width: the floats of a row of `values`, the context's D for every voice but one (render_graph_passes).
template <class LAYOUT, class LAUNCH>
int render_passes(sots_ctx *ctx, const char *who, const float *values, uint32_t width, uint32_t num_rows, uint32_t hop, uint32_t flags,
                  uint32_t samples_per_pass, uint64_t cap, uint32_t state_words, float *out, uint64_t out_samples, LAYOUT layout, LAUNCH launch)
{
    const uint32_t N = ctx->N, D = ctx->D;
    const uint64_t covered = (uint64_t)(num_rows - 1u) * hop + N, want = out_samples < covered ? out_samples : covered;
    // A pass is limited by its scratch (cap) and by the rows of genes its samples look at: at most count / hop + 3 of them,
    // kContMaxValueFloats floats.
    uint64_t pass = samples_per_pass ? samples_per_pass : cap;
    const uint64_t by_rows = (uint64_t)(kContMaxValueFloats / D - 3u) * hop;
    pass = pass > cap ? cap : pass;
    pass = pass > by_rows ? by_rows : pass;
    pass = pass > want ? (want ? want : 1u) : pass;
    auto ps = layout((uint32_t)pass);
    const size_t max_rows = (size_t)(pass / hop) + 3u;
    hipError_t e = render_reserve(ctx->render, max_rows * D, 0, ps.lay.stride);
    if (e == hipSuccess) e = render_reserve_words(ctx->render, ps.lay.words);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return SOTS_FAIL(ctx, SOTS_ERR_HIP, "%s: scratch allocation failed: %s", who, hipGetErrorString(e));
    }
    // every operator starts at phase 0 (a feedback operator with h1 = h2 = +0); a pass leaves its end state for the next one
    SOTS_HIP(ctx, hipMemsetAsync(ctx->render.words + ps.lay.carry, 0, state_words * sizeof(uint32_t), ctx->stream));
    ps.values = ctx->render.values, ps.wavetable = ctx->wavetable, ps.words = ctx->render.words, ps.out = ctx->render.out;
    ps.num_rows = num_rows, ps.hop = hop, ps.half_n = N / 2u, ps.glide = flags & SOTS_RENDER_GLIDE;
    ps.sp = ctx->sp;
    for (uint64_t s0 = 0; s0 < want; s0 += pass) {
        const uint32_t count = (uint32_t)(want - s0 < pass ? want - s0 : pass);
        uint32_t k0, k1, r;
        cont_position((uint32_t)s0, N / 2u, hop, num_rows, k0, r);
        cont_position((uint32_t)s0 + count - 1u, N / 2u, hop, num_rows, k1, r);
        k1 = k1 + 1u < num_rows ? k1 + 1u : num_rows - 1u; // (the row after: the second half of a hop, the far end of a glide)
        SOTS_HIP(ctx, hipMemcpyAsync(ctx->render.values, values + (size_t)k0 * width, (size_t)(k1 - k0 + 1u) * width * sizeof(float),
                                     hipMemcpyHostToDevice, ctx->stream));
        ps.row_base = k0, ps.n0 = (uint32_t)s0, ps.count = count;
        SOTS_HIP(ctx, launch(ps, k1 - k0 + 1u));
        // (stream order keeps the next pass off the scratch until this copy has read it)
        SOTS_HIP(ctx, hipMemcpyAsync(out + s0, ctx->render.out, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (out_samples > covered) memset(out + covered, 0, (size_t)(out_samples - covered) * sizeof(float));
    return SOTS_OK;
}

// the operator-graph voice: the flagged operators (beta != 0, or the index a gene), their B_j and the form of each one's
// chain.  None flagged: no chain launch, and hist, behind the eight carries, is neither cleared nor touched.
// With gene operators (sots_render_graph_genes alone gets here with any) a row of `values` is D = 2 OPS + E floats, and the
// track is split on the host before the first pass: the rows' first 2 OPS floats, which go to the device as the rows of every
// graph voice do, so that reduce, apply and mix are the kernels of every graph voice; and their E gene columns, which a pass
// puts behind its rows on the device for the chains (GraphGenes).  Both parts of a pass's rows fit the D floats per row that
// render_passes reserves.
int render_graph_passes(sots_ctx *ctx, const char *who, const float *values, uint32_t num_rows, uint32_t hop, uint32_t flags,
                        uint32_t samples_per_pass, uint32_t chain_form, uint32_t relax_cap, float *out, uint64_t out_samples)
{
    const uint32_t ops = ctx->graph.num_operators, D = ctx->D;
    GraphPass fb{};
    scale_feedback(ctx->feedback, ops, fb.scaled);
    const GraphGeneOps go = graph_gene_ops(ops, ctx->feedback_genes, ctx->feedback);
    fb.fb_mask = go.flagged;
    for (uint32_t j = 0; j < ops; ++j)
        if ((go.flagged >> j & 1u) && graph_genes_form(chain_form, go.genes >> j & 1u, ctx->feedback[j]) == kChainRelax) fb.forms |= 1u << j;
    fb.relax_cap = relax_cap ? relax_cap : kRelaxCapLibrary;
    GraphGenes gn{};
    gn.first = 2u * ops, gn.count = D - gn.first, gn.mask = go.genes;
    for (uint32_t j = 0; j < kGraphMaxOps; ++j) gn.column[j] = go.column[j];
    std::vector<float> split; // [num_rows][2 OPS], then [num_rows][E]; alive until the last pass's copies have been waited for
    const float *rows = values, *columns = nullptr;
    if (gn.mask) {
        split.resize((size_t)num_rows * D);
        float *front = split.data(), *back = front + (size_t)num_rows * gn.first;
        for (size_t r = 0; r < num_rows; ++r) {
            memcpy(front + r * gn.first, values + r * D, gn.first * sizeof(float));
            memcpy(back + r * gn.count, values + r * D + gn.first, gn.count * sizeof(float));
        }
        rows = front, columns = back;
    }
    const uint32_t flagged = (uint32_t)__builtin_popcount(fb.fb_mask);
    size_t behind = 0; // where the gene columns of a pass lie in the context's buffer of rows: behind the most rows a pass has
    const int rc = render_passes(
        ctx, who, rows, gn.first, num_rows, hop, flags, samples_per_pass, graph_feedback_max_pass(ops, flagged), fb.fb_mask ? 8u + 16u : 8u, out,
        out_samples,
        [&](uint32_t samples) {
            fb.lay = graph_layout(ops, flagged, samples);
            behind = ((size_t)(samples / hop) + 3u) * gn.first;
            return fb;
        },
        [&](const GraphPass &ps, uint32_t pass_rows) {
            if (!gn.mask) return launch_graph_pass(ctx->stream, ctx->graph, ctx->waveforms, ps, ctx->num_cus);
            gn.rows = ctx->render.values + behind;
            if (hipError_t e = hipMemcpyAsync(ctx->render.values + behind, columns + (size_t)ps.row_base * gn.count,
                                              (size_t)pass_rows * gn.count * sizeof(float), hipMemcpyHostToDevice, ctx->stream))
                return e;
            return launch_graph_pass(ctx->stream, ctx->graph, ctx->waveforms, ps, ctx->num_cus, &gn);
        });
    if (rc != SOTS_OK && gn.mask) (void)hipStreamSynchronize(ctx->stream); // (a copy out of `split` may still be under way)
    return rc;
}

} // namespace

// =======================================================================================
extern "C" {

// sots_create (graph == nullptr), sots_create_graph (feedback_genes == 0) and sots_create_graph_genes
static int create_context(const sots_config *cfg, const sots_voice_graph *graph, uint32_t feedback_genes, sots_ctx **out)
{
    *out = nullptr;
    SOTS_REFUSE(nullptr, config_check(*cfg, 1ull << 26, graph, feedback_genes));

    sots_ctx *ctx = new sots_ctx();
    // audio rows are padded off the power-of-two stride (see sots_kernels.h)
    uint32_t pad = 32;
#ifdef SOTS_EXPERIMENT
    if (const char *e = getenv("SOTS_AUDIO_PAD")) pad = (uint32_t)strtoul(e, nullptr, 10) & ~3u; // floats
    if (const char *e = getenv("SOTS_SYNTH_CUT")) ctx->allow_cut = atoi(e) != 0;                 // 0: never cut the chain
    if (const char *e = getenv("SOTS_FUSE_VARIATION")) ctx->fuse_variation = atoi(e) != 0 ? 1 : 0;
    if (const char *e = getenv("SOTS_SKIP_STAGE")) ctx->skip_stage = atoi(e); // 1: no synthesis, 2: no spectral kernel (timing ablations)
#endif
    if (int rc = engine_create(*ctx, *cfg, graph, pad, feedback_genes)) return abandon(ctx, rc);
#define CREATE_HIP(call) SOTS_HIP_OR(ctx, call, return abandon(ctx, rc_))
    const size_t pd_bytes = (size_t)2 * ctx->P * ctx->D * sizeof(float);
    const size_t audio_bytes = (size_t)ctx->P * ctx->pitch * sizeof(float);
    const size_t spec_bytes = (size_t)ctx->P * (ctx->N + 8) * sizeof(float);
    CREATE_HIP(hipMalloc((void **)&ctx->values, pd_bytes));
    CREATE_HIP(hipMalloc((void **)&ctx->steps, pd_bytes));
    CREATE_HIP(hipMalloc((void **)&ctx->fitness, (size_t)2 * ctx->P * sizeof(float)));
    CREATE_HIP(hipMalloc((void **)&ctx->audio, audio_bytes));
    CREATE_HIP(hipMalloc((void **)&ctx->spectrum, spec_bytes));
    CREATE_HIP(hipMalloc((void **)&ctx->target, (size_t)(ctx->N / 2) * sizeof(float)));
    CREATE_HIP(hipMalloc((void **)&ctx->keys, sort_keys_bytes(ctx->P)));
    {
        const size_t a = sort_scratch_bytes(ctx->P), b = select_scratch_bytes(ctx->P);
        CREATE_HIP(hipMalloc(&ctx->sort_scratch, a > b ? a : b));
    }
    CREATE_HIP(hipMalloc((void **)&ctx->splitters, 2 * select_splitter_slot_bytes()));
    CREATE_HIP(hipMemsetAsync(ctx->splitters, 0, 2 * select_splitter_slot_bytes(), ctx->stream));
    CREATE_HIP(hipMalloc((void **)&ctx->sel_cnt, 2 * select_counters_bytes()));
    CREATE_HIP(hipMemsetAsync(ctx->sel_cnt, 0, 2 * select_counters_bytes(), ctx->stream));
    CREATE_HIP(hipMalloc((void **)&ctx->sel_lists, select_lists_bytes(ctx->num_cus)));
    CREATE_HIP(hipMemsetAsync(ctx->sel_lists, 0, select_lists_bytes(ctx->num_cus), ctx->stream));
    if (const char *e = getenv("SOTS_SELECT_LISTS")) ctx->use_lists = strcmp(e, "0") != 0; // 0: the selection streams the fitness (comparisons)
    if (const char *e = getenv("SOTS_SELECT_PLAN")) { // one library measured both ways; sots_set_select_plan overrides it
        if (!strcmp(e, "tiles") || !strcmp(e, "1")) ctx->select_plan = SOTS_SELECT_TILES;
        else if (!strcmp(e, "splitters") || !strcmp(e, "2")) ctx->select_plan = SOTS_SELECT_SPLITTERS;
    }
    CREATE_HIP(hipMemsetAsync(ctx->values, 0, pd_bytes, ctx->stream));
    CREATE_HIP(hipMemsetAsync(ctx->steps, 0, pd_bytes, ctx->stream));
    CREATE_HIP(hipMemsetAsync(ctx->fitness, 0, (size_t)2 * ctx->P * sizeof(float), ctx->stream));
    CREATE_HIP(hipMemsetAsync(ctx->audio, 0, audio_bytes, ctx->stream));
    CREATE_HIP(hipMemsetAsync(ctx->spectrum, 0, spec_bytes, ctx->stream));
    CREATE_HIP(hipMemsetAsync(ctx->target, 0, (size_t)(ctx->N / 2) * sizeof(float), ctx->stream));
    TableStaging staging;
    if (int rc = engine_upload_tables(*ctx, staging)) return abandon(ctx, rc);
    CREATE_HIP(hipStreamSynchronize(ctx->stream));
#undef CREATE_HIP
    *out = ctx;
    return SOTS_OK;
}

int sots_create(const sots_config *cfg, sots_ctx **out)
{
    if (!cfg || !out) return SOTS_FAIL(nullptr, SOTS_ERR_INVALID, "sots_create: null argument");
    return create_context(cfg, nullptr, 0, out);
}

int sots_create_graph(const sots_config *cfg, const sots_voice_graph *graph, sots_ctx **out)
{
    if (!cfg || !graph || !out) return SOTS_FAIL(nullptr, SOTS_ERR_INVALID, "sots_create_graph: null argument");
    return create_context(cfg, graph, 0, out);
}

int sots_create_graph_genes(const sots_config *cfg, const sots_voice_graph *graph, uint32_t feedback_genes, sots_ctx **out)
{
    if (!cfg || !graph || !out) return SOTS_FAIL(nullptr, SOTS_ERR_INVALID, "sots_create_graph_genes: null argument");
    return create_context(cfg, graph, feedback_genes, out);
}

int sots_get_voice_feedback_genes(const sots_ctx *ctx, uint32_t *feedback_genes)
{
    SOTS_REQUIRE_CTX(ctx);
    return engine_get_voice_feedback_genes(*ctx, feedback_genes);
}

int sots_set_graph_synth_form(sots_ctx *ctx, uint32_t form)
{
    SOTS_REQUIRE_CTX(ctx);
    return engine_set_graph_synth_form(*ctx, form);
}

int sots_get_graph_synth_form(const sots_ctx *ctx, uint32_t *requested, uint32_t *effective)
{
    SOTS_REQUIRE_CTX(ctx);
    return engine_get_graph_synth_form(*ctx, ctx->P, requested, effective);
}

// pure host code: the plan rule of sots_rules.h
int sots_graph_time_parallel_capacity(const sots_voice_graph *graph, uint32_t *individuals_per_workgroup, uint32_t *levels)
{
    if (const Fault f = voice_graph_check(graph)) return SOTS_FAIL(nullptr, f.code, "%s", f.text);
    const GraphTpPlan plan = graph_tp_plan(*graph);
    if (individuals_per_workgroup) *individuals_per_workgroup = plan.capacity;
    if (levels) *levels = plan.levels;
    return SOTS_OK;
}

int sots_get_voice_graph(const sots_ctx *ctx, sots_voice_graph *graph)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!graph) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "sots_get_voice_graph: null argument");
    if (ctx->cfg.synth_kind != SOTS_SYNTH_GRAPH) return SOTS_FAIL(ctx, SOTS_ERR_STATE, "sots_get_voice_graph: the context runs a fixed voice (synth_kind %u)", ctx->cfg.synth_kind);
    *graph = ctx->graph;
    return SOTS_OK;
}

void sots_destroy(sots_ctx *ctx) { free_ctx(ctx); }

const char *sots_last_error(const sots_ctx *ctx) { return err_of(ctx).c_str(); }

int sots_set_stream(sots_ctx *ctx, void *hip_stream)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = engine_bind(*ctx)) return rc;
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return SOTS_OK;
}

int sots_synchronize(sots_ctx *ctx)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = engine_bind(*ctx)) return rc;
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SOTS_OK;
}

// ---- target ---------------------------------------------------------------------------
int sots_set_target_spectrum(sots_ctx *ctx, const float *magnitudes, uint32_t num_bins)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!magnitudes || num_bins != ctx->N / 2)
        return SOTS_FAIL(ctx, SOTS_ERR_SIZE, "target spectrum needs %u bins, got %u", ctx->N / 2, num_bins);
    if (int rc = engine_bind(*ctx)) return rc;
    SOTS_HIP(ctx, hipMemcpyAsync(ctx->target, magnitudes, (size_t)num_bins * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = derive_target(ctx)) return rc;
    ctx->target_set = true;
    return SOTS_OK;
}

int sots_set_target_audio(sots_ctx *ctx, const float *audio, uint32_t num_samples)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!audio || num_samples < ctx->N)
        return SOTS_FAIL(ctx, SOTS_ERR_SIZE, "target audio needs %u samples, got %u", ctx->N, num_samples);
    const std::vector<float> mag = target_spectrum(audio, ctx->N, ctx->window64, ctx->window_factor);
    return sots_set_target_spectrum(ctx, mag.data(), ctx->N / 2);
}

// ---- population -------------------------------------------------------------------------
int sots_init_population(sots_ctx *ctx, uint32_t chunk_index)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = engine_bind(*ctx)) return rc;
    ctx->rot = 0; // initPopulationCL, ...OpenCL.hpp:371
    ctx->generation = 0;
    // a tail the last run's selection left pending belongs to the OLD population: dropped, never completed into the new one
    ctx->tail_pending = false;
    ctx->tail_first = 0;
    ctx->spl_valid = false;
    ctx->lists_ready = false;
    ctx->next_exchange_set = false;
    SOTS_HIP(ctx, track_clear(ctx->track, ctx->stream));
    {
        StageScope t(ctx, SOTS_STAGE_INIT);
        SOTS_HIP(ctx, launch_init_population(ctx->stream, ctx->val(0), ctx->stp(0), ctx->fit(0), ctx->pd, chunk_index));
    }
    return maybe_drain(ctx);
}

static int copy_population(sots_ctx *ctx, uint32_t half, bool to_device, void *values, size_t values_bytes,
                           void *steps, size_t steps_bytes, void *fitness, size_t fitness_bytes)
{
    SOTS_REFUSE(ctx, population_bytes_check(ctx->P, ctx->D, values, values_bytes, steps, steps_bytes, fitness, fitness_bytes));
    if (int rc = engine_bind(*ctx)) return rc;
    const hipMemcpyKind kind = to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    auto cp = [&](void *host, void *dev, size_t bytes) {
        return to_device ? hipMemcpyAsync(dev, host, bytes, kind, ctx->stream)
                         : hipMemcpyAsync(host, dev, bytes, kind, ctx->stream);
    };
    if (values) SOTS_HIP(ctx, cp(values, ctx->val(half), values_bytes));
    if (steps) SOTS_HIP(ctx, cp(steps, ctx->stp(half), steps_bytes));
    if (fitness) SOTS_HIP(ctx, cp(fitness, ctx->fit(half), fitness_bytes));
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SOTS_OK;
}

int sots_write_population(sots_ctx *ctx, const float *values, size_t values_bytes, const float *steps,
                          size_t steps_bytes, const float *fitness, size_t fitness_bytes)
{
    SOTS_REQUIRE_CTX(ctx);
    // refused before anything changes: settle_tail ends a pending state, which under SOTS_SORT_TOP_ONLY cannot come back
    SOTS_REFUSE(ctx, population_bytes_check(ctx->P, ctx->D, values, values_bytes, steps, steps_bytes, fitness, fitness_bytes));
    if (int rc = settle_tail(ctx)) return rc;
    return copy_population(ctx, ctx->rot, true, (void *)values, values_bytes, (void *)steps, steps_bytes,
                           (void *)fitness, fitness_bytes);
}

int sots_read_population(sots_ctx *ctx, float *values, size_t values_bytes, float *steps, size_t steps_bytes,
                         float *fitness, size_t fitness_bytes)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = complete_tail(ctx)) return rc;
    return copy_population(ctx, ctx->rot, false, values, values_bytes, steps, steps_bytes, fitness, fitness_bytes);
}

int sots_read_population_other(sots_ctx *ctx, float *values, size_t values_bytes, float *steps,
                               size_t steps_bytes, float *fitness, size_t fitness_bytes)
{
    SOTS_REQUIRE_CTX(ctx);
    return copy_population(ctx, ctx->rot ^ 1u, false, values, values_bytes, steps, steps_bytes, fitness, fitness_bytes);
}

// ---- synthesiser buffers ---------------------------------------------------------------
int sots_write_synth(sots_ctx *ctx, const float *audio, size_t audio_bytes, const float *spectrum,
                     size_t spectrum_bytes)
{
    SOTS_REQUIRE_CTX(ctx);
    const size_t a_bytes = (size_t)ctx->P * ctx->N * sizeof(float), s_bytes = (size_t)ctx->P * (ctx->N + 8) * sizeof(float);
    if ((audio && audio_bytes != a_bytes) || (spectrum && spectrum_bytes != s_bytes))
        return SOTS_FAIL(ctx, SOTS_ERR_SIZE, "synth byte counts must be %zu (audio) and %zu (spectrum)", a_bytes, s_bytes);
    if (int rc = engine_bind(*ctx)) return rc;
    if (audio)
        SOTS_HIP(ctx, hipMemcpy2DAsync(ctx->audio, (size_t)ctx->pitch * sizeof(float), audio, (size_t)ctx->N * sizeof(float),
                                       (size_t)ctx->N * sizeof(float), ctx->P, hipMemcpyHostToDevice, ctx->stream));
    if (spectrum) SOTS_HIP(ctx, hipMemcpyAsync(ctx->spectrum, spectrum, s_bytes, hipMemcpyHostToDevice, ctx->stream));
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SOTS_OK;
}

int sots_read_synth(sots_ctx *ctx, float *audio, size_t audio_bytes, float *spectrum, size_t spectrum_bytes,
                    float *target, size_t target_bytes)
{
    SOTS_REQUIRE_CTX(ctx);
    const size_t a_bytes = (size_t)ctx->P * ctx->N * sizeof(float), s_bytes = (size_t)ctx->P * (ctx->N + 8) * sizeof(float);
    const size_t t_bytes = (size_t)(ctx->N / 2) * sizeof(float);
    if ((audio && audio_bytes != a_bytes) || (spectrum && spectrum_bytes != s_bytes) || (target && target_bytes != t_bytes))
        return SOTS_FAIL(ctx, SOTS_ERR_SIZE, "synth byte counts must be %zu (audio), %zu (spectrum), %zu (target)",
                    a_bytes, s_bytes, t_bytes);
    if (int rc = engine_bind(*ctx)) return rc;
    if (audio)
        SOTS_HIP(ctx, hipMemcpy2DAsync(audio, (size_t)ctx->N * sizeof(float), ctx->audio, (size_t)ctx->pitch * sizeof(float),
                                       (size_t)ctx->N * sizeof(float), ctx->P, hipMemcpyDeviceToHost, ctx->stream));
    if (spectrum) SOTS_HIP(ctx, hipMemcpyAsync(spectrum, ctx->spectrum, s_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (target) SOTS_HIP(ctx, hipMemcpyAsync(target, ctx->target, t_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SOTS_OK;
}

// ---- stages -------------------------------------------------------------------------------
int sots_stage_recombine(sots_ctx *ctx)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = settle_tail(ctx)) return rc;
    if (int rc = engine_bind(*ctx)) return rc;
    const uint32_t src = ctx->rot, dst = ctx->rot ^ 1u;
    {
        StageScope t(ctx, SOTS_STAGE_RECOMBINE);
        SOTS_HIP(ctx, launch_recombine(ctx->stream, ctx->val(src), ctx->stp(src), ctx->val(dst), ctx->stp(dst), ctx->pd));
    }
    ctx->rot = dst; // out-of-place recombination: the recombined population is the current one
    return maybe_drain(ctx);
}

int sots_stage_mutate(sots_ctx *ctx)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = settle_tail(ctx)) return rc;
    if (int rc = engine_bind(*ctx)) return rc;
    {
        StageScope t(ctx, SOTS_STAGE_MUTATE);
        SOTS_HIP(ctx, launch_mutate(ctx->stream, ctx->val(ctx->rot), ctx->stp(ctx->rot), ctx->pd, ctx->mc, ctx->generation));
    }
    return maybe_drain(ctx);
}

int sots_stage_synthesise(sots_ctx *ctx)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = settle_tail(ctx)) return rc;
    if (int rc = engine_bind(*ctx)) return rc;
    {
        StageScope t(ctx, SOTS_STAGE_SYNTHESISE);
        SOTS_HIP(ctx, engine_synthesise(*ctx, ctx->val(ctx->rot), ctx->audio, ctx->P, nullptr, ctx->allow_cut));
    }
    return maybe_drain(ctx);
}

int sots_stage_window(sots_ctx *ctx)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = settle_tail(ctx)) return rc;
    if (int rc = engine_bind(*ctx)) return rc;
    {
        StageScope t(ctx, SOTS_STAGE_WINDOW);
        SOTS_HIP(ctx, launch_window(ctx->stream, ctx->audio, ctx->window, ctx->P, ctx->log2n, ctx->pitch));
    }
    return maybe_drain(ctx);
}

int sots_stage_fft(sots_ctx *ctx)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = settle_tail(ctx)) return rc;
    if (int rc = engine_bind(*ctx)) return rc;
    {
        StageScope t(ctx, SOTS_STAGE_FFT);
        SOTS_HIP(ctx, launch_fft(ctx->stream, ctx->audio, ctx->spectrum, ctx->twiddle, ctx->P, ctx->log2n, ctx->pitch, ctx->num_cus, &ctx->occ));
    }
    return maybe_drain(ctx);
}

int sots_stage_fitness(sots_ctx *ctx)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = settle_tail(ctx)) return rc;
    if (int rc = require_target(ctx)) return rc;
    if (int rc = engine_bind(*ctx)) return rc;
    {
        StageScope t(ctx, SOTS_STAGE_FITNESS);
        SOTS_HIP(ctx, launch_fitness(ctx->stream, ctx->spectrum, fitness_target(ctx), ctx->fit(ctx->rot), ctx->P, ctx->log2n,
                                     ctx->inv_n, ctx->inv_wf, ctx->num_cus, &ctx->occ, ctx->obj));
    }
    return maybe_drain(ctx);
}

int sots_stage_sort(sots_ctx *ctx)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = settle_tail(ctx)) return rc;
    if (int rc = engine_bind(*ctx)) return rc;
    const uint32_t src = ctx->rot, dst = ctx->rot ^ 1u;
    {
        StageScope t(ctx, SOTS_STAGE_SORT);
        SOTS_HIP(ctx, launch_sort(ctx->stream, ctx->val(src), ctx->stp(src), ctx->fit(src), ctx->val(dst), ctx->stp(dst),
                                  ctx->fit(dst), ctx->keys, ctx->sort_scratch, ctx->P, ctx->D));
    }
    return maybe_drain(ctx);
}

int sots_stage_select(sots_ctx *ctx)
{
    SOTS_REQUIRE_CTX(ctx);
    const bool lists = ctx->lists_ready; // (filed from the half this selection reads, after its tail had been completed)
    if (int rc = settle_tail(ctx)) return rc;
    if (int rc = engine_bind(*ctx)) return rc;
    const uint32_t src = ctx->rot, dst = ctx->rot ^ 1u, need = selected_rows(ctx);
    if (ctx->sort_mode == SOTS_SORT_FULL || !select_applies(ctx->P, need)) return sots_stage_sort(ctx);
    {
        StageScope t(ctx, SOTS_STAGE_SORT);
        if (int rc = run_select(ctx, src, dst, need, nullptr, lists)) return rc;
    }
    ctx->tail_pending = true; // completed from the current (unsorted) half once sots_stage_rotate has flipped
    ctx->tail_first = 0;      // marks "selected into the other half, not rotated yet"
    return maybe_drain(ctx);
}

// files the keys of the current half's fitness between the splitters the next sots_stage_select reads, as the fused
// loop's spectral kernel does (tests: any fitness pattern and any slot reach the selection's list mode)
int sots_stage_bucket_fitness(sots_ctx *ctx)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!lists_possible(ctx)) return SOTS_FAIL(ctx, SOTS_ERR_STATE, "no key lists here: %u splitters per slot, SOTS_SELECT_LISTS=%d", select_splitter_count(ctx->num_cus), (int)ctx->use_lists);
    if (int rc = engine_bind(*ctx)) return rc;
    // it looks at every row's fitness: the rows a lazy selection left out are produced first (the sots_stage_select that
    // follows would produce them AFTER their stale fitness had been filed)
    if (int rc = complete_tail(ctx)) return rc;
    SelLists sl;
    if (int rc = open_lists(ctx, &sl)) return rc;
    SOTS_HIP(ctx, launch_bucket_fitness(ctx->stream, ctx->fit(ctx->rot), ctx->P, sl));
    ctx->lists_ready = true;
    return SOTS_OK;
}

// what sots_stage_bucket_fitness filed, as it lies in device memory (tests of the filing itself)
int sots_read_select_lists(sots_ctx *ctx, uint32_t *counts, uint32_t counts_len, uint64_t *keys, uint32_t keys_len)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!lists_possible(ctx) || !ctx->lists_ready) return SOTS_FAIL(ctx, SOTS_ERR_STATE, "no keys filed: sots_stage_bucket_fitness comes first");
    const uint32_t b = select_splitter_count(ctx->num_cus);
    if (!counts || !keys || counts_len != b * kSelListShards || keys_len != b * kSelListCap)
        return SOTS_FAIL(ctx, SOTS_ERR_SIZE, "select lists: %u counters and %u keys needed, got %u and %u", b * kSelListShards, b * kSelListCap, counts_len, keys_len);
    if (int rc = engine_bind(*ctx)) return rc;
    SOTS_HIP(ctx, hipMemcpyAsync(counts, counter_set(ctx, ctx->spl_cur), (size_t)counts_len * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    SOTS_HIP(ctx, hipMemcpyAsync(keys, ctx->sel_lists, (size_t)keys_len * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SOTS_OK;
}

int sots_stage_rotate(sots_ctx *ctx)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = engine_bind(*ctx)) return rc;
    ctx->lists_ready = false; // (filed from what was the current half)
    // rotationIndex_ flip, ...OpenCL.hpp:486; a kernel argument here, so no transfer
    StageScope t(ctx, SOTS_STAGE_ROTATE);
    if (ctx->tail_pending && ctx->tail_first == 0) { // sots_stage_select just ran: its rows are in the OTHER half
        ctx->tail_first = selected_rows(ctx);
    } else if (ctx->tail_pending) {
        if (int rc = settle_tail(ctx)) return rc; // (the flip below would swap the halves under a pending state)
    }
    ctx->rot ^= 1u;
    ctx->generation += 1;
    return SOTS_OK;
}

int sots_execute_generation(sots_ctx *ctx)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = require_target(ctx)) return rc;
    int rc;
    if ((rc = sots_stage_recombine(ctx))) return rc;
    if ((rc = sots_stage_mutate(ctx))) return rc;
    if ((rc = sots_stage_synthesise(ctx))) return rc;
    if ((rc = sots_stage_window(ctx))) return rc;
    if ((rc = sots_stage_fft(ctx))) return rc;
    if ((rc = sots_stage_fitness(ctx))) return rc;
    if ((rc = sots_stage_sort(ctx))) return rc;
    if ((rc = sots_stage_rotate(ctx))) return rc;
    return record_generation(ctx);
}

int sots_execute_generations(sots_ctx *ctx, uint32_t n)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = require_target(ctx)) return rc;
    if (int rc = engine_bind(*ctx)) return rc;
    if (ctx->tail_pending && ctx->tail_first == 0)
        return SOTS_FAIL(ctx, SOTS_ERR_STATE, "sots_stage_select must be followed by sots_stage_rotate");
    const uint32_t need = selected_rows(ctx);
    const bool select = ctx->sort_mode != SOTS_SORT_FULL && select_applies(ctx->P, need);
    // an exchange folded into the last generation's sort (sots_fuse_exchange_next_sort) is used once
    const SortExchange exchange = ctx->next_exchange;
    const bool with_exchange = ctx->next_exchange_set && n > 0;
    hipEvent_t gate = with_exchange ? ctx->next_exchange_gate : nullptr;
    if (n > 0) ctx->next_exchange_set = false, ctx->next_exchange_gate = nullptr;
    if (with_exchange && select && exchange.sink && exchange.sink_rows > need)
        return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "fused exchange: %u elite rows asked for, sortPopulation places %u per generation here", exchange.sink_rows, need);
    ctx->lists_ready = false;
    for (uint32_t g = 0; g < n; ++g) {
        // the variation below overwrites the unsorted half a pending tail would be completed from; nobody has
        // asked for those rows, so they are dropped
        ctx->tail_pending = false;
        ctx->chain_tail = nullptr; // (the caller may have put other work on the stream since the last generation)
        uint32_t src = ctx->rot, dst = ctx->rot ^ 1u;
        // Large populations of 4-gene individuals make their individuals inside the synthesis kernel
        // (one launch less, 151 vs 157 us per generation at P = 65536); with few wavefronts per CU or
        // more genes the serial per-lane variation costs more than the launch it saves (measured).
        const bool device_arith = ctx->synth_arith == SOTS_ARITH_DEVICE_KERNELS; // (compatibility kernel: makes no individuals)
        const bool graph_voice = ctx->cfg.synth_kind == SOTS_SYNTH_GRAPH;        // (its kernel makes no individuals either)
        const bool fuse_variation = device_arith || graph_voice ? false : ctx->fuse_variation >= 0 ? ctx->fuse_variation == 1
                                                             : (ctx->pd.d <= 4 && ctx->P >= 192u * (ctx->num_cus ? ctx->num_cus : 256u)) ||
                                                                   // a few individuals per CU: k_synth_tp makes them, a thread per gene
                                                                   (ctx->allow_cut && synth_time_parallel(ctx->cfg.synth_kind, ctx->P, ctx->num_cus)) ||
                                                                   // small populations of the 2- and 3-operator voices: the cut kernel's helper wavefronts (launch_synth);
                                                                   // with 8 genes it is a draw (204 = 204 us at P = 1024, 373 against 368 at 32768)
                                                                   (ctx->pd.d <= 6 && ctx->cfg.synth_kind != SOTS_SYNTH_TRIPLE_PAR && ctx->allow_cut && ctx->P <= 128u * (ctx->num_cus ? ctx->num_cus : 256u)) ||
                                                                   // 3- and 4-operator voices from 65 individuals per CU: k_synth_ol (round 4) makes its workgroup's
                                                                   // individuals first, a thread per gene, whatever the number of genes
                                                                   (ctx->allow_cut && synth_operators_in_lanes(ctx->cfg.synth_kind, ctx->P, ctx->num_cus));
        if (!fuse_variation) {
            StageScope t(ctx, SOTS_STAGE_FUSED_VARIATION, true);
            SOTS_HIP(ctx, launch_recombine_mutate(ctx->stream, ctx->val(src), ctx->stp(src), ctx->val(dst), ctx->stp(dst),
                                                  ctx->pd, ctx->mc, ctx->generation));
        }
        ctx->rot = dst;
        if (ctx->skip_stage != 1) {
            StageScope t(ctx, SOTS_STAGE_FUSED_SYNTH, true);
            // raw synthesis (the window is applied by the FFT kernel as it loads the row); by default the
            // kernel also makes its individuals: recombination + mutation from the sorted half
            sots::Variation var = {ctx->val(src), ctx->stp(src), ctx->val(dst), ctx->stp(dst), ctx->pd, ctx->mc, ctx->generation};
            SOTS_HIP(ctx, engine_synthesise(*ctx, ctx->val(ctx->rot), ctx->audio, ctx->P, fuse_variation ? &var : nullptr, ctx->allow_cut));
        }
        // Will this generation's selection be the one-launch one, in front of the wide N = 1024 spectral kernel?  Then that
        // kernel files every row's key under its bucket, and the selection reads lists instead of all P fitness values.
        const bool lists = select && use_splitters(ctx) && lists_in_loop(ctx);
        if (ctx->skip_stage != 2) {
            StageScope t(ctx, SOTS_STAGE_FUSED_SPECTRAL, true);
            SelLists sl;
            if (lists)
                if (int rc = open_lists(ctx, &sl)) return rc;
            SOTS_HIP(ctx, launch_fft_fitness(ctx->stream, ctx->audio, ctx->window, fitness_target(ctx), ctx->fit(ctx->rot), ctx->twiddle, ctx->P,
                                             ctx->log2n, ctx->pitch, ctx->inv_n, ctx->inv_wf, ctx->num_cus, &ctx->occ, lists ? &sl : nullptr, ctx->obj));
        }
        src = ctx->rot;
        dst = ctx->rot ^ 1u;
        const SortExchange *ex = with_exchange && g + 1 == n ? &exchange : nullptr;
        // The rows this sort takes were gathered on ANOTHER stream.  The host waits for that collective here, with this
        // generation's variation, synthesis and spectral kernels already on the stream (the GPU stays busy, and the
        // collective - started a generation ago - is normally long done), instead of making the stream wait: on this
        // runtime a cross-stream event wait costs the waiting stream ~18 us even when the event is complete
        // (tools/ubench/cross_stream.hip).  A kernel launched after the host has seen the event sees the rows.
        // In front of the sort's StageScope: a host wait is not sort-kernel time.
        if (ex && gate) SOTS_HIP(ctx, hipEventSynchronize(gate));
        {
            StageScope t(ctx, SOTS_STAGE_SORT, true);
            if (select) {
                // the rows recombination reads, in order; the rest of the order is produced on demand
                if (int rc = run_select(ctx, src, dst, need, ex, lists)) return rc;
            } else {
                SOTS_HIP(ctx, launch_sort(ctx->stream, ctx->val(src), ctx->stp(src), ctx->fit(src), ctx->val(dst), ctx->stp(dst),
                                          ctx->fit(dst), ctx->keys, ctx->sort_scratch, ctx->P, ctx->D, 0, ex));
            }
        }
        ctx->rot = dst;
        ctx->tail_pending = select;
        ctx->tail_first = need;
        ctx->generation += 1;
        if (int rc = record_generation(ctx)) return rc;
        if (int rc = maybe_drain(ctx)) return rc;
    }
    return SOTS_OK;
}

// ---- run record ---------------------------------------------------------------------------
int sots_track(sots_ctx *ctx, uint32_t flags, uint32_t history_every, uint32_t history_capacity)
{
    SOTS_REQUIRE_CTX(ctx);
    SOTS_REFUSE(ctx, track_args_check(&flags, history_every, history_capacity, 0));
    if (int rc = engine_bind(*ctx)) return rc;
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream)); // a record launch may still be using the old buffers
    SOTS_HIP(ctx, track_setup(ctx->track, flags, history_every, history_capacity, 1, ctx->stream));
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SOTS_OK;
}

int sots_read_best_ever(sots_ctx *ctx, float *values, size_t values_bytes, float *steps, size_t steps_bytes, float *fitness,
                        uint32_t *generation)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!ctx->track.best_ever()) return SOTS_FAIL(ctx, SOTS_ERR_STATE, "best-ever tracking is off: call sots_track first");
    const size_t d_bytes = (size_t)ctx->D * sizeof(float);
    if ((values && values_bytes != d_bytes) || (steps && steps_bytes != d_bytes))
        return SOTS_FAIL(ctx, SOTS_ERR_SIZE, "best-ever byte counts must be %zu (values, steps)", d_bytes);
    if (int rc = engine_bind(*ctx)) return rc;
    if (values) SOTS_HIP(ctx, hipMemcpyAsync(values, ctx->track.rows, d_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (steps) SOTS_HIP(ctx, hipMemcpyAsync(steps, ctx->track.rows + SOTS_MAX_DIMS, d_bytes, hipMemcpyDeviceToHost, ctx->stream));
    SOTS_HIP(ctx, track_fetch_meta(ctx->track, ctx->stream, 1));
    if (fitness) *fitness = track_fitness(ctx->track, 0);
    if (generation) *generation = ctx->track.pinned[1];
    return SOTS_OK;
}

int sots_read_history(sots_ctx *ctx, sots_gen_record *out, uint32_t capacity, uint32_t *written, uint64_t *taken)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!ctx->track.history()) return SOTS_FAIL(ctx, SOTS_ERR_STATE, "the history is off: call sots_track with SOTS_TRACK_HISTORY first");
    if (!written || (capacity && !out)) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "read_history: null argument");
    if (int rc = engine_bind(*ctx)) return rc;
    SOTS_HIP(ctx, track_read_history(ctx->track, ctx->stream, 0, out, capacity, written));
    if (taken) *taken = ctx->track.taken;
    return SOTS_OK;
}

int sots_stop_rule_holds(const sots_stop_rule *rule, float best_ever_fitness, uint32_t best_ever_generation, uint32_t generation)
{
    if (int rc = stop_rule_check(rule)) return rc;
    // (one copy of the arithmetic for the host and for the chunk queue's turnover kernel: sots_stop_rule.h)
    return stop_rule_holds(rule->target_fitness, rule->stall_generations, best_ever_fitness, best_ever_generation, generation) ? 1 : 0;
}

int sots_execute_until(sots_ctx *ctx, uint32_t max_generations, const sots_stop_rule *rule, uint32_t *generations_run)
{
    SOTS_REQUIRE_CTX(ctx);
    if (generations_run) *generations_run = 0;
    if (stop_rule_check(rule)) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "stop rule: null, wrong struct_size or check_interval 0");
    if (!ctx->track.best_ever()) return SOTS_FAIL(ctx, SOTS_ERR_STATE, "sots_execute_until needs best-ever tracking: call sots_track first");
    uint32_t done = 0;
    while (done < max_generations) {
        const uint32_t block = std::min(rule->check_interval, max_generations - done);
        if (int rc = sots_execute_generations(ctx, block)) return rc;
        done += block;
        if (generations_run) *generations_run = done;
        SOTS_HIP(ctx, track_fetch_meta(ctx->track, ctx->stream, 1));
        if (sots_stop_rule_holds(rule, track_fitness(ctx->track, 0), ctx->track.pinned[1], ctx->generation) == 1) break;
    }
    return SOTS_OK;
}

int sots_set_sort_mode(sots_ctx *ctx, uint32_t mode)
{
    SOTS_REQUIRE_CTX(ctx);
    if (mode > SOTS_SORT_TOP_ONLY) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "unknown sort mode %u", mode);
    // the new mode decides what happens to a pending tail: leaving SOTS_SORT_TOP_ONLY completes it (the unsorted half
    // is intact as long as the state is pending, settle_tail), entering it keeps the rows unspecified
    ctx->sort_mode = mode;
    ctx->spl_valid = false;
    ctx->lists_ready = false;
    return complete_tail(ctx);
}

int sots_set_select_plan(sots_ctx *ctx, uint32_t plan)
{
    SOTS_REQUIRE_CTX(ctx);
    if (plan > SOTS_SELECT_SPLITTERS) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "unknown select plan %u", plan);
    ctx->select_plan = plan;
    ctx->lists_ready = false;
    return SOTS_OK;
}

int sots_select_splitter_count(const sots_ctx *ctx, uint32_t *count)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!count) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "null count");
    *count = select_splitter_count(ctx->num_cus);
    return SOTS_OK;
}

int sots_write_select_splitters(sots_ctx *ctx, const uint64_t *keys, uint32_t count)
{
    SOTS_REQUIRE_CTX(ctx);
    const uint32_t b = select_splitter_count(ctx->num_cus);
    if (!keys || count != b) return SOTS_FAIL(ctx, SOTS_ERR_SIZE, "select splitters: %u keys needed, got %u", b, count);
    if (int rc = engine_bind(*ctx)) return rc;
    ctx->lists_ready = false; // (filed between the old splitters)
    SOTS_HIP(ctx, hipMemcpyAsync(splitter_slot(ctx, ctx->spl_cur), keys, (size_t)b * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SOTS_OK;
}

int sots_read_select_splitters(sots_ctx *ctx, uint64_t *keys, uint32_t count)
{
    SOTS_REQUIRE_CTX(ctx);
    const uint32_t b = select_splitter_count(ctx->num_cus);
    if (!keys || count != b) return SOTS_FAIL(ctx, SOTS_ERR_SIZE, "select splitters: %u keys needed, got %u", b, count);
    if (int rc = engine_bind(*ctx)) return rc;
    SOTS_HIP(ctx, hipMemcpyAsync(keys, splitter_slot(ctx, ctx->spl_cur), (size_t)b * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SOTS_OK;
}

int sots_set_synth_arithmetic(sots_ctx *ctx, uint32_t arith)
{
    SOTS_REQUIRE_CTX(ctx);
    return engine_set_synth_arithmetic(*ctx, arith);
}

// A setting, like the sort mode: it changes what the NEXT variation computes and nothing now - a pending lazy tail stays
// pending (rows 0..numParents-1, all that variation takes survivors from, are placed whatever the tail's state).
int sots_set_survivors(sots_ctx *ctx, uint32_t n)
{
    SOTS_REQUIRE_CTX(ctx);
    return engine_set_survivors(*ctx, n);
}

int sots_get_survivors(const sots_ctx *ctx, uint32_t *n)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!n) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "null survivors pointer");
    *n = ctx->pd.survivors;
    return SOTS_OK;
}

// Like a new target (derive_target): same population, another landscape.  A pending lazy tail is an order under the OLD
// fitness values, which stay in place until the next evaluation: it is kept, as sots_set_target_* keeps it.
int sots_set_objective(sots_ctx *ctx, uint32_t objective, float floor)
{
    SOTS_REQUIRE_CTX(ctx);
    Objective old;
    if (int rc = engine_set_objective(*ctx, objective, floor, &old)) return rc;
    if (int rc = derive_target(ctx)) {
        engine_restore_objective(*ctx, old);
        return rc;
    }
    return SOTS_OK;
}

// Like a new objective: another landscape for the same population.  Everything is checked before anything changes.
int sots_set_objective_weights(sots_ctx *ctx, const float *weights, uint32_t num_bins)
{
    SOTS_REQUIRE_CTX(ctx);
    Objective old;
    if (int rc = engine_set_objective_weights(*ctx, weights, num_bins, &old)) return rc;
    if (int rc = derive_target(ctx)) {
        engine_restore_objective(*ctx, old);
        return rc;
    }
    if (weights) ctx->weights_w.assign(weights, weights + num_bins);
    else ctx->weights_w.clear();
    return SOTS_OK;
}

// Like a new objective: another landscape for the same population - the run record, the stored splitters and the key lists
// say nothing under the new voice.  The target's images do not depend on the voice and stay.  Everything is checked, and
// the record cleared, before the setting changes.
int sots_set_voice_waveforms(sots_ctx *ctx, const uint32_t *codes, uint32_t count)
{
    SOTS_REQUIRE_CTX(ctx);
    SOTS_REFUSE(ctx, voice_waveforms_check(ctx->cfg.synth_kind, ctx->graph.num_operators, codes, count));
    if (int rc = engine_bind(*ctx)) return rc;
    SOTS_HIP(ctx, track_clear(ctx->track, ctx->stream));
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->spl_valid = false;
    ctx->lists_ready = false;
    return engine_set_voice_waveforms(*ctx, codes, count);
}

int sots_get_voice_waveforms(const sots_ctx *ctx, uint32_t codes[8])
{
    SOTS_REQUIRE_CTX(ctx);
    return engine_get_voice_waveforms(*ctx, codes);
}

// ... and so is a new feedback setting
int sots_set_voice_feedback(sots_ctx *ctx, const float *index, uint32_t count)
{
    SOTS_REQUIRE_CTX(ctx);
    SOTS_REFUSE(ctx, voice_feedback_check(ctx->cfg.synth_kind, ctx->graph.num_operators, index, count, ctx->feedback_genes));
    if (int rc = engine_bind(*ctx)) return rc;
    SOTS_HIP(ctx, track_clear(ctx->track, ctx->stream));
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->spl_valid = false;
    ctx->lists_ready = false;
    return engine_set_voice_feedback(*ctx, index, count);
}

int sots_get_voice_feedback(const sots_ctx *ctx, float index[8])
{
    SOTS_REQUIRE_CTX(ctx);
    return engine_get_voice_feedback(*ctx, index);
}

int sots_get_objective_weights(const sots_ctx *ctx, float *weights, uint32_t num_bins, uint32_t *is_set)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!weights && !is_set) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "null weights and is_set pointers");
    if (weights && num_bins != ctx->N / 2) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "objective weights have %u bins, room for %u", ctx->N / 2, num_bins);
    if (is_set) *is_set = ctx->weights_w.empty() ? 0u : 1u;
    if (weights && !ctx->weights_w.empty()) std::copy(ctx->weights_w.begin(), ctx->weights_w.end(), weights);
    return SOTS_OK;
}

int sots_get_objective(const sots_ctx *ctx, uint32_t *objective, float *floor)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!objective && !floor) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "null objective and floor pointers");
    if (objective) *objective = ctx->obj.kind;
    if (floor) *floor = ctx->obj.floor;
    return SOTS_OK;
}

int sots_get_generation(const sots_ctx *ctx, uint32_t *generation)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!generation) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "null generation pointer");
    *generation = ctx->generation;
    return SOTS_OK;
}

int sots_set_generation(sots_ctx *ctx, uint32_t generation)
{
    SOTS_REQUIRE_CTX(ctx);
    ctx->generation = generation;
    return SOTS_OK;
}

// ---- overlap-add rendering ----------------------------------------------------
int sots_render_overlap_add(sots_ctx *ctx, const float *values, size_t values_bytes, uint32_t num_rows, const sots_render_args *args,
                            float *out, uint64_t out_samples)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!args || args->struct_size != sizeof(sots_render_args))
        return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "sots_render_overlap_add: null args or sots_render_args.struct_size != %zu", sizeof(sots_render_args));
    const uint32_t N = ctx->N, hop = args->hop;
    if (hop < (N + 63u) / 64u || hop > N)
        return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "sots_render_overlap_add: hop %u outside %u..%u", hop, (N + 63u) / 64u, N);
    if (args->flags & ~(uint32_t)SOTS_RENDER_WINDOWED) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "sots_render_overlap_add: unknown flags 0x%x", args->flags);
    if (num_rows == 0) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "sots_render_overlap_add: num_rows must be at least 1");
    if (!values || values_bytes != (size_t)num_rows * ctx->D * sizeof(float))
        return SOTS_FAIL(ctx, SOTS_ERR_SIZE, "sots_render_overlap_add: %u rows need %zu bytes of values, got %zu", num_rows,
                    (size_t)num_rows * ctx->D * sizeof(float), values_bytes);
    if (!out && out_samples) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "sots_render_overlap_add: null output");
    if (int rc = engine_bind(*ctx)) return rc;

    // A pass takes `step` chunk starts of output and holds, besides those chunks, the `reach` chunks in front of them that
    // extend into its range: synthesised again, so a pass needs nothing of the pass before it.
    const uint32_t reach = (N + hop - 1u) / hop - 1u, cap = render_max_rows(ctx->pitch);
    uint32_t step = args->rows_per_pass ? args->rows_per_pass : 4096u;
    step = step > cap ? cap : step;
    step = step > num_rows ? num_rows : step;
    const uint64_t covered = (uint64_t)(num_rows - 1u) * hop + N, want = out_samples < covered ? out_samples : covered;
    const size_t max_rows = (size_t)step + reach;
    // (the synthesis kernels store whole tiles of rows where a tile is full: a margin of one tile behind the last row)
    if (hipError_t e = render_reserve(ctx->render, max_rows * ctx->D, (max_rows + 64u) * ctx->pitch, (size_t)step * hop + N + 4u)) {
        (void)hipGetLastError();
        return SOTS_FAIL(ctx, SOTS_ERR_HIP, "sots_render_overlap_add: scratch allocation failed: %s", hipGetErrorString(e));
    }
    for (uint32_t r0 = 0; r0 < num_rows && (uint64_t)r0 * hop < want; r0 += step) {
        const uint32_t r1 = num_rows - r0 > step ? r0 + step : num_rows, first = r0 > reach ? r0 - reach : 0u, rows = r1 - first;
        const uint64_t s0 = (uint64_t)r0 * hop, s1 = r1 == num_rows ? want : (uint64_t)r1 * hop, end = s1 < want ? s1 : want;
        const uint32_t count = (uint32_t)(end - s0);
        SOTS_HIP(ctx, hipMemcpyAsync(ctx->render.values, values + (size_t)first * ctx->D, (size_t)rows * ctx->D * sizeof(float),
                                     hipMemcpyHostToDevice, ctx->stream));
        SOTS_HIP(ctx, engine_synthesise(*ctx, ctx->render.values, ctx->render.audio, rows, nullptr, ctx->allow_cut));
        RenderPass ps{};
        ps.audio = ctx->render.audio;
        ps.window = (args->flags & SOTS_RENDER_WINDOWED) ? ctx->window : nullptr;
        ps.out = ctx->render.out;
        ps.rows = rows, ps.hop = hop, ps.n = N, ps.pitch = ctx->pitch;
        ps.out_first = (r0 - first) * hop;
        ps.quads = (count + 3u) / 4u;
        SOTS_HIP(ctx, launch_overlap_add(ctx->stream, ps));
        // (stream order keeps the next pass off the scratch until this copy has read it)
        SOTS_HIP(ctx, hipMemcpyAsync(out + s0, ctx->render.out, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    }
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (out_samples > covered) memset(out + covered, 0, (size_t)(out_samples - covered) * sizeof(float));
    return SOTS_OK;
}

// ---- phase-continuous rendering --------------------------------------
int sots_render_continuous(sots_ctx *ctx, const float *values, size_t values_bytes, uint32_t num_rows, const sots_render_continuous_args *args,
                           float *out, uint64_t out_samples)
{
    SOTS_REQUIRE_CTX(ctx);
    SOTS_REFUSE(ctx, render_continuous_voice_check(ctx->cfg.synth_kind));
    SOTS_REFUSE(ctx, render_continuous_check(args, ctx->N, ctx->D, ctx->synth_arith, values, values_bytes, num_rows, out, out_samples));
    if (int rc = engine_bind(*ctx)) return rc;
    const uint32_t kind = ctx->cfg.synth_kind;
    return render_passes(
        ctx, "sots_render_continuous", values, ctx->D, num_rows, args->hop, args->flags, args->samples_per_pass, kContMaxPass, kContMaxStages * kContMaxChains,
        out, out_samples,
        [&](uint32_t samples) {
            ContPass ps{};
            ps.lay = cont_layout(kind, samples);
            return ps;
        },
        [&](const ContPass &ps, uint32_t) { return launch_continuous_pass(ctx->stream, kind, ps, ctx->num_cus); });
}

int sots_render_graph_continuous(sots_ctx *ctx, const float *values, size_t values_bytes, uint32_t num_rows,
                                 const sots_render_continuous_args *args, float *out, uint64_t out_samples)
{
    SOTS_REQUIRE_CTX(ctx);
    SOTS_REFUSE(ctx, render_graph_continuous_check(ctx->cfg.synth_kind, ctx->feedback, args, ctx->N, ctx->D, values, values_bytes, num_rows, out,
                                                   out_samples, ctx->feedback_genes));
    if (int rc = engine_bind(*ctx)) return rc;
    // (the check has seen to it that no operator is flagged)
    return render_graph_passes(ctx, "sots_render_graph_continuous", values, num_rows, args->hop, args->flags, args->samples_per_pass, 0, 0, out,
                               out_samples);
}

int sots_render_graph_feedback(sots_ctx *ctx, const float *values, size_t values_bytes, uint32_t num_rows,
                               const sots_render_graph_feedback_args *args, float *out, uint64_t out_samples)
{
    SOTS_REQUIRE_CTX(ctx);
    SOTS_REFUSE(ctx, render_graph_feedback_check(ctx->cfg.synth_kind, args, ctx->N, ctx->D, values, values_bytes, num_rows, out, out_samples,
                                                 ctx->feedback_genes));
    if (int rc = engine_bind(*ctx)) return rc;
    return render_graph_passes(ctx, "sots_render_graph_feedback", values, num_rows, args->hop, args->flags, args->samples_per_pass, args->chain_form,
                               args->relax_cap, out, out_samples);
}

int sots_render_graph_genes(sots_ctx *ctx, const float *values, size_t values_bytes, uint32_t num_rows, const sots_render_graph_feedback_args *args,
                            float *out, uint64_t out_samples)
{
    SOTS_REQUIRE_CTX(ctx);
    SOTS_REFUSE(ctx, render_graph_genes_check(ctx->cfg.synth_kind, args, ctx->N, ctx->D, values, values_bytes, num_rows, out, out_samples));
    if (int rc = engine_bind(*ctx)) return rc;
    return render_graph_passes(ctx, "sots_render_graph_genes", values, num_rows, args->hop, args->flags, args->samples_per_pass, args->chain_form,
                               args->relax_cap, out, out_samples);
}

// ---- timing ----------------------------------------------------------------------------------
int sots_timing_enable(sots_ctx *ctx, int enabled)
{
    SOTS_REQUIRE_CTX(ctx);
    ctx->timing = enabled != 0;
    return SOTS_OK;
}

int sots_timing_reset(sots_ctx *ctx)
{
    SOTS_REQUIRE_CTX(ctx);
    if (int rc = engine_bind(*ctx)) return rc;
    if (int rc = drain_clocks(ctx)) return rc;
    for (auto &ck : ctx->clocks) {
        ck.total_ms = 0.0;
        ck.count = 0;
        ck.launches_ms.clear();
    }
    return SOTS_OK;
}

int sots_stage_time_ms(sots_ctx *ctx, int stage, double *total_ms, uint64_t *count)
{
    SOTS_REQUIRE_CTX(ctx);
    if (stage < 0 || stage >= SOTS_STAGE_COUNT) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "stage %d out of range", stage);
    if (int rc = engine_bind(*ctx)) return rc;
    if (int rc = drain_clocks(ctx)) return rc;
    if (total_ms) *total_ms = ctx->clocks[stage].total_ms;
    if (count) *count = ctx->clocks[stage].count;
    return SOTS_OK;
}

int sots_stage_launch_times_ms(sots_ctx *ctx, int stage, float *out_ms, uint64_t capacity, uint64_t *written)
{
    SOTS_REQUIRE_CTX(ctx);
    if (stage < 0 || stage >= SOTS_STAGE_COUNT) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "stage %d out of range", stage);
    if (!written || (capacity && !out_ms)) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "stage_launch_times: null argument");
    if (int rc = engine_bind(*ctx)) return rc;
    if (int rc = drain_clocks(ctx)) return rc;
    const std::vector<float> &v = ctx->clocks[stage].launches_ms;
    const uint64_t n = v.size() < capacity ? v.size() : capacity;
    for (uint64_t i = 0; i < n; ++i) out_ms[i] = v[i];
    *written = n;
    return SOTS_OK;
}

// ---- island exchange ------------------------------------------------------------------------
int sots_pack_elites_device(sots_ctx *ctx, void *device_rows, uint32_t n_rows)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!device_rows || n_rows > ctx->P) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "pack_elites: bad rows/n_rows %u", n_rows);
    if (ctx->tail_pending && n_rows > ctx->tail_first) {
        if (ctx->sort_mode == SOTS_SORT_TOP_ONLY)
            return SOTS_FAIL(ctx, SOTS_ERR_STATE, "pack_elites: %u rows asked for, SOTS_SORT_TOP_ONLY placed %u", n_rows, ctx->tail_first);
        if (int rc = complete_tail(ctx)) return rc;
    }
    if (int rc = engine_bind(*ctx)) return rc;
    SOTS_HIP(ctx, launch_pack_rows(ctx->stream, ctx->val(ctx->rot), ctx->stp(ctx->rot), ctx->fit(ctx->rot),
                                   (float *)device_rows, 0, n_rows, ctx->D));
    return SOTS_OK;
}

int sots_inject_immigrants_device(sots_ctx *ctx, const void *device_rows, uint32_t n_rows)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!device_rows || n_rows > breeding_rows(ctx))
        return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "inject_immigrants: %u rows do not fit the %u parent rows recombination reads", n_rows, breeding_rows(ctx));
    if (int rc = engine_bind(*ctx)) return rc;
    SOTS_HIP(ctx, launch_unpack_rows(ctx->stream, ctx->val(ctx->rot), ctx->stp(ctx->rot), ctx->fit(ctx->rot),
                                     (const float *)device_rows, breeding_rows(ctx) - n_rows, n_rows, ctx->D, 0, 0));
    return SOTS_OK;
}

int sots_inject_gathered_device(sots_ctx *ctx, const void *gathered_rows, uint32_t world, uint32_t rank, uint32_t elites)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!gathered_rows || world == 0 || rank >= world)
        return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "inject_gathered: bad arguments (world %u, rank %u)", world, rank);
    const uint64_t n_rows = (uint64_t)(world - 1) * elites;
    if (n_rows > breeding_rows(ctx))
        return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "inject_gathered: %llu immigrant rows do not fit the %u parent rows recombination reads",
                    (unsigned long long)n_rows, breeding_rows(ctx));
    if (int rc = engine_bind(*ctx)) return rc;
    SOTS_HIP(ctx, launch_unpack_rows(ctx->stream, ctx->val(ctx->rot), ctx->stp(ctx->rot), ctx->fit(ctx->rot),
                                     (const float *)gathered_rows, breeding_rows(ctx) - (uint32_t)n_rows, (uint32_t)n_rows,
                                     ctx->D, rank * elites, elites));
    return SOTS_OK;
}

int sots_fuse_exchange_next_sort(sots_ctx *ctx, void *elite_rows, uint32_t n_elite_rows, const void *gathered_rows,
                                 uint32_t world, uint32_t rank, uint32_t elites, void *host_gate_event)
{
    SOTS_REQUIRE_CTX(ctx);
    ctx->next_exchange_set = false;
    ctx->next_exchange_gate = nullptr;
    SortExchange ex{};
    if (elite_rows) {
        if (n_elite_rows == 0 || n_elite_rows > ctx->P) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "fused exchange: bad elite row count %u", n_elite_rows);
        ex.sink = (float *)elite_rows;
        ex.sink_rows = n_elite_rows;
    }
    if (gathered_rows) {
        if (world == 0 || rank >= world) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "fused exchange: bad arguments (world %u, rank %u)", world, rank);
        const uint64_t n_rows = (uint64_t)(world - 1) * elites;
        if (n_rows > breeding_rows(ctx))
            return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "fused exchange: %llu immigrant rows do not fit the %u parent rows recombination reads",
                        (unsigned long long)n_rows, breeding_rows(ctx));
        if (n_rows) {
            ex.imm = (const float *)gathered_rows;
            ex.imm_first = breeding_rows(ctx) - (uint32_t)n_rows;
            ex.imm_rows = (uint32_t)n_rows;
            ex.skip_first = rank * elites;
            ex.skip_count = elites;
        }
    }
    if (!ex.sink && !ex.imm) return SOTS_OK; // nothing to fold in
    ctx->next_exchange = ex;
    ctx->next_exchange_set = true;
    ctx->next_exchange_gate = (hipEvent_t)host_gate_event;
    return SOTS_OK;
}

int sots_pack_elites_host(sots_ctx *ctx, float *rows, uint32_t n_rows)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!rows) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "pack_elites: null rows");
    if (int rc = engine_bind(*ctx)) return rc;
    if (int rc = ensure_rows(ctx, n_rows)) return rc;
    if (int rc = sots_pack_elites_device(ctx, ctx->rows, n_rows)) return rc;
    SOTS_HIP(ctx, hipMemcpyAsync(rows, ctx->rows, (size_t)n_rows * (2 * ctx->D + 1) * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SOTS_OK;
}

int sots_inject_immigrants_host(sots_ctx *ctx, const float *rows, uint32_t n_rows)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!rows) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "inject_immigrants: null rows");
    if (int rc = engine_bind(*ctx)) return rc;
    if (int rc = ensure_rows(ctx, n_rows)) return rc;
    SOTS_HIP(ctx, hipMemcpyAsync(ctx->rows, rows, (size_t)n_rows * (2 * ctx->D + 1) * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (int rc = sots_inject_immigrants_device(ctx, ctx->rows, n_rows)) return rc;
    SOTS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SOTS_OK;
}

int sots_get_info(const sots_ctx *ctx, sots_info *info)
{
    SOTS_REQUIRE_CTX(ctx);
    if (!info) return SOTS_FAIL(ctx, SOTS_ERR_INVALID, "null info");
    memset(info, 0, sizeof *info);
    info->population_length = ctx->P;
    info->num_dimensions = ctx->D;
    info->audio_length = ctx->N;
    info->spectrum_row_floats = ctx->N + 8;
    info->rotation_index = ctx->rot;
    info->generation = ctx->generation;
    info->compute_units = ctx->num_cus;
    snprintf(info->device_name, sizeof info->device_name, "%s", ctx->device_name);
    snprintf(info->arch, sizeof info->arch, "%s", ctx->arch);
    return SOTS_OK;
}

} // extern "C"
