/*
 * sots_hip.h -- C-ABI of libsots_hip.so, the MI355X (gfx950) backend for the
 * per-generation evolutionary FM sound-matching loop.
 *
 * This is the drop-in boundary: Evolutionary_Strategy_HIP (C++, host/) and the
 * ctypes binding (capi.py) sit on top of exactly these entry points.  Plain
 * pointers and sizes only; no C++ or torch types cross it.  One context is used
 * from one host thread at a time (the reference's objects are single-threaded
 * too).  Every call returns SOTS_OK (0) or a negative code;
 * sots_last_error() gives the text.  All file:line citations are relative to the
 * reference tree.
 *
 * Population state, as in the reference's device buffer set
 * (Evolutionary_Strategy_OpenCL.hpp:60-63,278-292):
 *   value, step : float[2][P][D]   two rotation halves, one row per individual
 *   fitness     : float[2][P]
 *   audio       : float[P][N]
 *   spectrum    : float[P][N+8]    interleaved complex, N/2+4 bins per row,
 *                                  bins 0..N/2 valid (clFFT layout, :164-168)
 *   target      : float[N/2]
 * P = numParents + numOffspring, D = numDimensions, N = 2^audioLengthLog2.
 */
#ifndef SOTS_HIP_H
#define SOTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOTS_MAX_DIMS 16
#define SOTS_WAVETABLE_SIZE 32768u /* Evolutionary_Strategy.hpp:197 */
#define SOTS_SAMPLE_RATE 44100u    /* Evolutionary_Strategy.hpp:196 */

enum sots_status {
    SOTS_OK = 0,
    SOTS_ERR_INVALID = -1,   /* bad argument / unsupported configuration */
    SOTS_ERR_HIP = -2,       /* a HIP runtime call failed */
    SOTS_ERR_NO_DEVICE = -3, /* no usable gfx950 device */
    SOTS_ERR_SIZE = -4,      /* caller buffer too small / wrong byte count */
    SOTS_ERR_STATE = -5      /* call out of order (e.g. no target set) */
};

/* Which FM voice synthesisePopulation runs; numDimensions must match. */
enum sots_synth_kind {
    SOTS_SYNTH_2OP = 0,        /* D=4,  ocl_program.cl:280-330, Evolutionary_Strategy.hpp:368-402 */
    SOTS_SYNTH_3OP_SERIES = 1, /* D=6,  ocl_program.cl:332-386, Evolutionary_Strategy.hpp:403-449 */
    SOTS_SYNTH_TRIPLE_PAR = 2, /* D=12, ocl_program.cl:388-443, Evolutionary_Strategy.hpp:450-495 */
    SOTS_SYNTH_4OP_SERIES = 3, /* D=8,  build-defined 4-operator series chain (BASELINE config 4) */
    SOTS_SYNTH_GRAPH = 4       /* D=2*OPS, an operator graph given at creation: sots_voice_graph below */
};

/* Stage ids, in the order of the reference's kernelNames_
 * (Evolutionary_Strategy_OpenCL.hpp:54,117). */
enum sots_stage {
    SOTS_STAGE_INIT = 0,
    SOTS_STAGE_RECOMBINE = 1,
    SOTS_STAGE_MUTATE = 2,
    SOTS_STAGE_SYNTHESISE = 3,
    SOTS_STAGE_WINDOW = 4,
    SOTS_STAGE_FFT = 5,
    SOTS_STAGE_FITNESS = 6,
    SOTS_STAGE_SORT = 7,
    SOTS_STAGE_ROTATE = 8,
    /* kernels of the fused generation loop (sots_execute_generations) */
    SOTS_STAGE_FUSED_VARIATION = 9, /* recombine + mutate */
    SOTS_STAGE_FUSED_SYNTH = 10,    /* synthesise */
    SOTS_STAGE_FUSED_SPECTRAL = 11, /* window + FFT + fitness */
    SOTS_STAGE_SORT_TAIL = 12,      /* the rest of the order after a selection, produced when it is read */
    SOTS_STAGE_COUNT = 13
};

/* What sortPopulation delivers inside sots_execute_generations (and sots_stage_select).
 * The next generation's recombinePopulation reads whole parent blocks only (ocl_program.cl:99-112),
 * i.e. rows 0..S-1 of the sorted half, S = max(numParents, max(1, numParents/workgroupSize)*workgroupSize). */
enum sots_sort_mode {
    SOTS_SORT_LAZY_TAIL = 0, /* default: each generation places rows 0..S-1, in order and bit-identical to the full
                              * sort; rows S..P-1 are produced, from the still intact unsorted half, by the first
                              * call that looks at them (read/write population, any sots_stage_*, packing more
                              * than S elites).  A population outside 1024 < P <= 131072 or with S > P/2 is sorted in full.
                              * Calls that WRITE rows (stages, write_population, init) end the pending state.
                              * Settings (target, objective, weights, survivors, arithmetic, voice, select plan, splitters,
                              * sots_set_generation, sots_track), the renderers, sots_inject_immigrants_* (the rows it writes
                              * are placed rows) and every refused call neither produce nor drop the rows; a generation of
                              * either loop and sots_stage_recombine read rows 0..S-1 only and write every row anew. */
    SOTS_SORT_FULL = 1,      /* the reference's behaviour: every generation sorts all P rows
                              * (ocl_program.cl:664-711, Evolutionary_Strategy.hpp:108-124) */
    SOTS_SORT_TOP_ONLY = 2   /* like 0 but rows S..P-1 are never produced (their content is unspecified; packing more
                              * than S elites fails with SOTS_ERR_STATE) */
};

/* How the selection of rows 0..S-1 (modes 0 and 2 above) is computed; the rows are the same bit for bit.
 * TILES: two launches, sorted 1024-key tiles and a rank pass over their prefixes.  SPLITTERS: one launch that ranks every
 * key between stored 64-bit splitters - exact whatever they are, fast when they are the previous selection's (each
 * selection stores the next one's).  AUTO (default): SPLITTERS from the second generation of a run on, for P <= 65536,
 * and for P <= 131072 where the fused loop's spectral kernel files the keys for it (N = 1024);
 * TILES for the first generation after anything replaced rows, fitness, target or sort mode, and from sots_stage_select.
 * The environment variable SOTS_SELECT_PLAN (auto | tiles | splitters), read by sots_create, sets the initial plan. */
enum sots_select_plan { SOTS_SELECT_AUTO = 0, SOTS_SELECT_TILES = 1, SOTS_SELECT_SPLITTERS = 2 };

/* Which of the reference's two arithmetics synthesisePopulation uses.  Its CPU path (Evolutionary_Strategy.hpp:203,368-495)
 * keeps the sample-rate ratio in fp32; its device kernels (ocl_program.cl:280-443) write it as a double expression, fuse
 * their multiply-adds and, in the 3-op voice, add params[4] where the CPU path adds params[5]: the same parameters give
 * audio a few wavetable steps apart.  north_star names the CPU path as the parity target: the default,
 * and what every tuned kernel computes. */
enum sots_synth_arith {
    SOTS_ARITH_CPU_PATH = 0,
    SOTS_ARITH_DEVICE_KERNELS = 1 /* bit-identical to the reference's OpenCL kernels as compiled for this GPU
                                   * (tests/test_ocl_reference.py); one plain kernel, not tuned; not for the 4-op voice */
};

/* Replaces Evolutionary_Strategy_OpenCL_Arguments
 * (Evolutionary_Strategy_OpenCL.hpp:25-38) + Evolutionary_Strategy_Arguments
 * (Evolutionary_Strategy.hpp:579-589). */
typedef struct sots_config {
    uint32_t struct_size;       /* = sizeof(sots_config) */
    uint32_t num_parents;       /* es_args.pop.numParents */
    uint32_t num_offspring;     /* es_args.pop.numOffspring */
    uint32_t num_dimensions;    /* es_args.pop.numDimensions */
    uint32_t audio_length_log2; /* es_args.audioLengthLog2, 8..15 (N = 256 ... 32768; main.cpp:90 takes any) */
    uint32_t num_generations;   /* es_args.numGenerations */
    uint32_t synth_kind;        /* enum sots_synth_kind */
    uint32_t workgroup_size;    /* workgroupX: the recombination block (WRKGRPSIZE in ocl_program.cl:86-148) */
    int32_t device;             /* HIP device ordinal (replaces deviceType) */
    uint32_t gid_base;          /* global id of individual 0 (island offset for the PRNG) */
    uint64_t seed;              /* PRNG key (replaces the wall-clock seed, ...OpenCL.hpp:383) */
    float param_min[SOTS_MAX_DIMS]; /* es_args.paramMin */
    float param_max[SOTS_MAX_DIMS]; /* es_args.paramMax */
} sots_config;

typedef struct sots_ctx sots_ctx;

/* ---- lifetime (replaces Evolutionary_Strategy_OpenCL::init, ...OpenCL.hpp:138-150) ---- */
int sots_create(const sots_config *cfg, sots_ctx **out);
void sots_destroy(sots_ctx *ctx);
/* text of the last failure on ctx (or of the last failed sots_create when ctx == NULL) */
const char *sots_last_error(const sots_ctx *ctx);
/* run every later launch/copy on this hipStream_t (NULL = the context's own stream) */
int sots_set_stream(sots_ctx *ctx, void *hip_stream);
int sots_synchronize(sots_ctx *ctx);

/* ---- operator-graph voice (new: SOTS_SYNTH_GRAPH, user-defined feed-forward FM algorithms of 2 to 8 operators) ----
 * The topology travels beside sots_config (which cannot grow): cfg.synth_kind must be SOTS_SYNTH_GRAPH and
 * cfg.num_dimensions must be 2 * num_operators.  sots_create, sots_batch_create and sots_group_create refuse kind 4
 * (SOTS_ERR_INVALID; the text names sots_create_graph); islands do not take the voice.
 *
 * The voice.  OPS operators, 2 <= OPS <= 8, D = 2 OPS genes.
 * Genes and scaling:
 *   - Gene 2j is operator j's frequency f_j.  Gene 2j+1 is its level a_j.
 *   - Scaled per gene, as everywhere else: p_g = pmin_g + v_g (pmax_g - pmin_g), all fp32.
 *   - There is no `& 3` folding of the ranges as in the triple voice.
 * Topology:
 *   - modulators[j] is a bit mask.  Only bits i < j may be set.  Bit i set means operator i's output modulates
 *     operator j.  Feed-forward only: no operator modulates an earlier one or itself.  An operator's feedback onto its
 *     own phase is a setting of its own, not an edge of the graph: sots_set_voice_feedback, below.
 *   - carriers is a bit mask and is not empty.
 *   - Every operator is exactly one of two things.  Either it is a carrier and modulates nobody, or it is not a carrier
 *     and modulates at least one operator.  Everything else is refused.
 * Per-operator values:
 *   - A_j = f_j a_j if j is a modulator.  Its output is a frequency deviation in Hz and a_j is the modulation index, as
 *     in the 2-op voice.
 *   - A_j = a_j if j is a carrier.
 *   - c = (float)W / (float)44100, with W the wavetable size.  All phases start at 0.
 * Per sample n, operators in ascending j:
 *   1. o_j = tab_at(pos_j) A_j.  tab_at is table[clamp((int)pos, 0, W-1)]: the index is clamped on the float, and NaN or
 *      a negative value gives entry 0.
 *   2. An unmodulated operator has cur = f_j.  A modulated one has cur = ((o_i1 + o_i2) + ...) + f_j, over the set bits
 *      in ascending i.  An operator whose bit is clear is skipped, not added as 0.
 *   3. pos_j += c cur.  Multiply, then add.  No contraction.
 *   4. If pos_j >= W, subtract W.  For a modulated operator only: if pos_j < 0, add W afterwards.  An unmodulated
 *      operator has no lower wrap.  This is the 2-op voice's rule.
 * Output of sample n:
 *   - audio[n] = ((o_c1 + o_c2) + ...) over the carriers in ascending j.
 *   - With more than one carrier, that sum is divided by (float)count with a correctly rounded fp32 division.
 * Anchors: the graph {0->1, carrier 1} is SOTS_SYNTH_2OP bit for bit, and {0->1, 2->3, 4->5, carriers 1, 3, 5}, with
 * the ranges of genes 0..3 repeated per pair, is SOTS_SYNTH_TRIPLE_PAR bit for bit.  The two series voices are NOT
 * reproduced by any graph: their genes mean something else (operator frequencies in genes 1, 3, 5, 7 and a carrier
 * amplitude that is the product of two genes).
 * Not for the voice: SOTS_ARITH_DEVICE_KERNELS (SOTS_ERR_INVALID, as for the 4-op voice) and sots_render_continuous
 * (SOTS_ERR_INVALID: its scans are written per fixed voice; sots_render_graph_continuous, below, is the voice's own
 * phase-continuous renderer).  sots_render_overlap_add and everything else serve it. */
typedef struct sots_voice_graph {
    uint32_t struct_size;   /* = sizeof(sots_voice_graph) */
    uint32_t num_operators; /* OPS, 2..8 */
    uint32_t carriers;      /* bit j: operator j is heard */
    uint32_t modulators[8]; /* [j] bit i (i < j): operator i modulates operator j; entries >= OPS are 0 */
} sots_voice_graph;
int sots_create_graph(const sots_config *cfg, const sots_voice_graph *graph, sots_ctx **out);
/* the context's graph; SOTS_ERR_STATE for a context of a fixed voice */
int sots_get_voice_graph(const sots_ctx *ctx, sots_voice_graph *graph);

/* ---- operator waveforms of the graph voice (new: shapes cut out of the one sine table, as OPL2/OPL3 and TX81Z do) ----
 * Every operator of a sots_voice_graph has a waveform code; all are SOTS_WAVE_SINE until set.  Step 1 of the voice
 * above becomes
 *     o_j = shape(w_j, i) A_j
 * with i the index tab_at uses, clamp((int)pos_j, 0, W-1) decided on the float (NaN and negatives give 0), W = 32768
 * and T the wavetable:
 *     0 SOTS_WAVE_SINE       T[i]
 *     1 SOTS_WAVE_HALF       i < W/2 ? T[i] : +0.0f
 *     2 SOTS_WAVE_ABS        fabsf(T[i])                       (the sign bit cleared)
 *     3 SOTS_WAVE_PULSE      (i & W/4) == 0 ? fabsf(T[i]) : +0.0f
 *     4 SOTS_WAVE_EVEN       i < W/2 ? T[2i] : +0.0f
 *     5 SOTS_WAVE_ABS_EVEN   i < W/2 ? fabsf(T[2i]) : +0.0f
 *     6 SOTS_WAVE_SQUARE     i < W/2 ? +1.0f : -1.0f
 *     7 SOTS_WAVE_SAW        (float)i * 2^-14 - 1.0f           (both operations exact in fp32 for i < 2^15)
 * Every case is decided on the integer index, never on the sign of a table entry (the table is sinf(i/(W-1) 2 pi): its
 * last entry is a tiny value of either sign).  The product with A_j is always formed: +0 x inf is NaN and +0 x negative
 * is -0.  Everything else in the voice - the sums from -0, the wraps, the carrier mean - is unchanged, and with all codes
 * 0 the voice is the one above bit for bit.
 * sots_set_voice_waveforms: codes[count], count == the graph's num_operators, every code < 8; (NULL, 0) sets all sine.
 * SOTS_ERR_STATE for a context of a fixed voice, SOTS_ERR_INVALID for the rest; everything is checked before anything
 * changes, and a refused call leaves the old setting.  A successful call acts like a new objective: the run record is
 * cleared, the stored selection splitters and key lists are dropped; the population stays.  It may come before or after
 * the target, the objective and the weights.  sots_get_voice_waveforms writes all eight codes (0 beyond the operators).
 * Islands (sots_group) do not take the voice and have no such setting. */
enum {
    SOTS_WAVE_SINE = 0, SOTS_WAVE_HALF = 1, SOTS_WAVE_ABS = 2, SOTS_WAVE_PULSE = 3,
    SOTS_WAVE_EVEN = 4, SOTS_WAVE_ABS_EVEN = 5, SOTS_WAVE_SQUARE = 6, SOTS_WAVE_SAW = 7
};
int sots_set_voice_waveforms(sots_ctx *ctx, const uint32_t *codes, uint32_t count);
int sots_get_voice_waveforms(const sots_ctx *ctx, uint32_t codes[8]);

/* ---- per-operator feedback of the graph voice (new: an operator's phase offset by its own output, as in hardware FM) ----
 * Every operator j of a sots_voice_graph has a feedback index beta_j, +0 until set, and keeps two more state words, h1_j
 * and h2_j, both +0 at sample 0.  For an operator with beta_j != 0, step 1 of the voice becomes, all fp32 and uncontracted:
 *     K   = 0x1.45f306p+12f                     (5215.18896484375, the fp32 nearest W / 2 pi)
 *     B_j = beta_j * K                          (one fp32 product)
 *     g   = (h1_j + h2_j) * 0.5f
 *     z   = pos_j + B_j * g                     (multiply, then add)
 *     if (z >= W) z -= W;  if (z < 0) z += W;   (in this order, once each)
 *     i   = clamp((int)z, 0, W-1) decided on the float, NaN and negatives to 0   (as for pos_j)
 *     t_j = shape(w_j, i);   o_j = t_j * A_j
 *     h2_j = h1_j;  h1_j = t_j
 * h is the shaped table value BEFORE the level: its magnitude is at most 1 for every shape, so with beta_j <= 2 one wrap
 * each way suffices for a phase in [0, W); any other phase is caught by the clamp, as it always was.  An operator with
 * beta_j == 0 is skipped: its index is that of pos_j, not of pos_j plus an offset of 0.  Steps 2 to 4 (increment, pos_j
 * update, wraps) and the carrier sum are untouched: feedback never changes pos_j and does not make an operator
 * "modulated" for the lower wrap.  With all beta zero the voice is the one above bit for bit.  Feedback combines freely
 * with the waveform codes and with any role.  The indices belong to the algorithm, like the codes: they are not evolved,
 * and the voice keeps its 2 num_operators genes (sots_create_graph_genes, below, makes chosen operators' indices genes).
 * sots_set_voice_feedback: index[count], count == the graph's num_operators, every index in [0, 2] (NaN, infinite,
 * negative and larger values are refused; -0 is taken as 0); (NULL, 0) sets all zero.  SOTS_ERR_STATE for a context of a
 * fixed voice, SOTS_ERR_INVALID for the rest; everything is checked before anything changes, and a refused call leaves
 * the old setting.  A successful call acts like sots_set_voice_waveforms: the run record is cleared, the stored selection
 * splitters and key lists are dropped; population and target stay.  In any order with target, objective, weights and
 * waveforms.  sots_get_voice_feedback writes all eight indices (0 beyond the operators).  Islands have no such setting;
 * sots_render_continuous and device-kernel arithmetic refuse the graph voice as before, and sots_render_graph_continuous
 * refuses a voice with any index != 0; sots_render_graph_feedback renders such a voice phase-continuously. */
int sots_set_voice_feedback(sots_ctx *ctx, const float *index, uint32_t count);
int sots_get_voice_feedback(const sots_ctx *ctx, float index[8]);

/* ---- feedback indices as genes (new: the matcher searches beta per individual) ----
 * sots_create_graph_genes is sots_create_graph with a mask feedback_genes: bit j set (j < OPS only) makes operator j's
 * feedback index a gene of the individual instead of a setting of the context.  Mask 0 is sots_create_graph in every
 * respect.
 * Gene layout.  E = popcount(feedback_genes); the voice has D = 2 OPS + E genes, D <= SOTS_MAX_DIMS, and
 * cfg.num_dimensions must be that D (the rule "kind 4 needs numDimensions 2 OPS" stays for sots_create_graph).  Genes
 * 0 .. 2 OPS - 1 mean what they mean above.  Gene 2 OPS + r holds the index of the operator with the r-th set bit of the
 * mask, ascending.  It is scaled like every gene, p = pmin_g + v (pmax_g - pmin_g) in fp32, and for these genes the
 * configuration must have 0 <= pmin_g <= pmax_g <= 2.
 * The effective index.  Mutation's reflection can leave v outside [0, 1], so the voice uses
 *     beta = p > 0 ? fminf(p, 2) : +0            (NaN, negative values and -0 give +0; values above 2 give 2)
 *     B    = beta * K                            (one fp32 product, as for the fixed setting)
 * A gene operator ALWAYS runs the feedback step of sots_set_voice_feedback, with its row's B: it is never "skipped", not
 * even where its beta is +0.  It keeps h1 and h2 and applies both wraps to z.  With pos_j in [0, W) and beta = +0, z is
 * pos_j and both wraps leave it: the index is that of pos_j, as for a skipped operator; a pos_j outside [0, W) (an
 * unmodulated operator of negative frequency, a NaN) meets the wraps of z before the clamp.  Everything else in the
 * voice is untouched.
 * Anchor: a row whose effective index is b on every gene operator gives the audio of sots_create_graph with
 * sots_set_voice_feedback = b on those operators, bit for bit, for b in (0, 2].
 * The other operators keep their setting: sots_set_voice_feedback refuses an index other than 0 on a gene operator
 * (SOTS_ERR_INVALID; nothing changes) and sots_get_voice_feedback reports 0 for it.  sots_get_voice_feedback_genes gives
 * the mask (0 for a context of sots_create_graph; SOTS_ERR_STATE for a fixed voice).
 * Refusals, all SOTS_ERR_INVALID and before any device work, each with a text of its own: a mask bit at or beyond OPS,
 * D > 16, cfg.num_dimensions != 2 OPS + E, a gene range outside [0, 2] or inverted.
 * Variation, selection, the run record, batch, queue, carried rows and survivors are generic in D and serve the voice;
 * sots_render_overlap_add and the match report render each row with its own beta.  sots_render_graph_continuous and
 * sots_render_graph_feedback take beta from the context and refuse a context whose mask is not 0 (SOTS_ERR_STATE; the
 * text names sots_render_overlap_add); sots_render_graph_genes renders such a voice phase-continuously, every row with its
 * own beta.  Islands do not take the voice. */
int sots_create_graph_genes(const sots_config *cfg, const sots_voice_graph *graph, uint32_t feedback_genes, sots_ctx **out);
int sots_get_voice_feedback_genes(const sots_ctx *ctx, uint32_t *feedback_genes);

/* The synthesis FORM of the operator-graph voice (new): which kernel computes the audio.  The three never
 * differ in a bit of any output - audio, fitness, populations, run record, rendered matches: every value sees the
 * operations of the definition above in the sample-by-sample order, unfused, in either kernel.
 *   LANES          a lane per individual (the only form until now): its time does not depend on how many lanes are alive.
 *   TIME_PARALLEL  the time axis in the lanes, for a few individuals per CU: per operator a wavefront that turns a block
 *                  of 64 increments into 64 phases, lane = individual, and one or two that evaluate everything else,
 *                  lane = sample.  A workgroup holds at most sots_graph_time_parallel_capacity() individuals; a larger
 *                  share of the rows is taken in several groups - correct, not necessarily fast.
 *   AUTO (default) TIME_PARALLEL where a CU's share of the rows of a launch fits one group and is at most the measured
 *                  limit, LANES elsewhere.
 * Whatever is requested, a voice with any feedback index other than 0 (sots_set_voice_feedback) or with feedback genes
 * (sots_create_graph_genes) runs LANES: a feedback operator's value is a serial chain through a table read.
 * sots_set_graph_synth_form clears nothing - not the run record, not the stored splitters, not the target.  It refuses a
 * fixed voice (SOTS_ERR_STATE) and an unknown code (SOTS_ERR_INVALID).  sots_get_graph_synth_form gives the request and
 * `effective`: what the next synthesis of the context's own population would launch, LANES or TIME_PARALLEL, recomputed
 * from the current state (either pointer may be NULL, not both). */
enum sots_graph_synth_form { SOTS_GRAPH_FORM_AUTO = 0, SOTS_GRAPH_FORM_LANES = 1, SOTS_GRAPH_FORM_TIME_PARALLEL = 2 };
int sots_set_graph_synth_form(sots_ctx *ctx, uint32_t form); /* enum sots_graph_synth_form */
int sots_get_graph_synth_form(const sots_ctx *ctx, uint32_t *requested, uint32_t *effective);
/* The individuals a workgroup of the TIME_PARALLEL form holds for this graph (0: the form does not take it) and the
 * graph's levels (0 for an unmodulated operator, else one more than its deepest modulator; the count is the largest + 1).
 * Either output may be NULL.  A malformed graph is refused with the graph rule's own text (sots_last_error(NULL)).  Pure
 * host code: no device, no handle. */
int sots_graph_time_parallel_capacity(const sots_voice_graph *graph, uint32_t *individuals_per_workgroup, uint32_t *levels);

/* ---- target (replaces setTargetAudio, ...OpenCL.hpp:563-570; Objective::calculateFFT,
 *      Evolutionary_Strategy.hpp:524-542) ---- */
int sots_set_target_audio(sots_ctx *ctx, const float *audio, uint32_t num_samples);
int sots_set_target_spectrum(sots_ctx *ctx, const float *magnitudes, uint32_t num_bins);

/* ---- population (initPopulationCL ...OpenCL.hpp:369-378; write/readPopulationData :403-430) ---- */
int sots_init_population(sots_ctx *ctx, uint32_t chunk_index);
/* any pointer may be NULL; byte counts must equal P*D*4 (values, steps) and P*4 (fitness).
 * Reads and writes address the CURRENT rotation half.  The byte counts are checked before anything changes: a refused
 * sots_write_population (SOTS_ERR_SIZE) leaves rows, pending state and stored splitters as they were. */
int sots_write_population(sots_ctx *ctx, const float *values, size_t values_bytes,
                          const float *steps, size_t steps_bytes,
                          const float *fitness, size_t fitness_bytes);
int sots_read_population(sots_ctx *ctx, float *values, size_t values_bytes,
                         float *steps, size_t steps_bytes,
                         float *fitness, size_t fitness_bytes);
/* the other rotation half (the reference's "output" arrays, main.cpp:241) */
int sots_read_population_other(sots_ctx *ctx, float *values, size_t values_bytes,
                               float *steps, size_t steps_bytes,
                               float *fitness, size_t fitness_bytes);

/* ---- synthesiser buffers (write/readSynthesizerData, ...OpenCL.hpp:436-453) ----
 * audio: P*N*4 bytes; spectrum: P*(N+8)*4 bytes; target: (N/2)*4 bytes; NULL skips. */
int sots_write_synth(sots_ctx *ctx, const float *audio, size_t audio_bytes,
                     const float *spectrum, size_t spectrum_bytes);
int sots_read_synth(sots_ctx *ctx, float *audio, size_t audio_bytes,
                    float *spectrum, size_t spectrum_bytes,
                    float *target, size_t target_bytes);

/* ---- the nine stages, one launch sequence each (executeGeneration, ...OpenCL.hpp:471-541) ---- */
int sots_stage_recombine(sots_ctx *ctx);
int sots_stage_mutate(sots_ctx *ctx);
int sots_stage_synthesise(sots_ctx *ctx);
int sots_stage_window(sots_ctx *ctx);
int sots_stage_fft(sots_ctx *ctx);
int sots_stage_fitness(sots_ctx *ctx);
int sots_stage_sort(sots_ctx *ctx);
/* the fused loop's sortPopulation as a stage: rows 0..S-1 only (enum sots_sort_mode); must be followed by
 * sots_stage_rotate.  Falls back to sots_stage_sort where the selection does not apply. */
int sots_stage_select(sots_ctx *ctx);
int sots_stage_rotate(sots_ctx *ctx);

/* stage-separated generation: the eight stages above in reference order */
int sots_execute_generation(sots_ctx *ctx);
/* n generations of the fused loop (recombine+mutate | synthesise | window+FFT+fitness |
 * sort | rotate); bit-identical population results to n x sots_execute_generation
 * (sortPopulation places the rows the next generation reads and leaves the rest of the order to
 * the first reader, enum sots_sort_mode).
 * The window is applied as the FFT kernel loads a row, so afterwards the audio buffer holds
 * the UN-windowed synthesis and the spectrum buffer is untouched.
 * Only enqueues - with ONE exception: after sots_fuse_exchange_next_sort with a host_gate_event the call blocks the
 * calling thread on that event (hipEventSynchronize) before it enqueues the last generation's sort, so the host never
 * runs more than the kernels of one generation ahead of a gathered exchange.
 * (executeAllGenerations, ...OpenCL.hpp:542-547) */
int sots_execute_generations(sots_ctx *ctx, uint32_t n);

/* enum sots_sort_mode.  The new mode decides what happens to rows a selection has left out: leaving SOTS_SORT_TOP_ONLY, or
 * SOTS_SORT_LAZY_TAIL for SOTS_SORT_FULL, while they are outstanding produces them now; entering SOTS_SORT_TOP_ONLY keeps them
 * outstanding (unspecified until the mode is left again).  Where a write has ended the pending state in between, leaving
 * SOTS_SORT_TOP_ONLY produces nothing: rows S..P-1 stay what the write left.  Setting the mode in force again changes nothing. */
int sots_set_sort_mode(sots_ctx *ctx, uint32_t mode);
int sots_set_select_plan(sots_ctx *ctx, uint32_t plan); /* enum sots_select_plan */
/* The splitters the next SPLITTERS selection reads (one per compute unit: sots_select_splitter_count), for tests and
 * diagnostics: keys are (order-preserving fitness bits << 32) | row index; any values are allowed. */
int sots_select_splitter_count(const sots_ctx *ctx, uint32_t *count);
int sots_write_select_splitters(sots_ctx *ctx, const uint64_t *keys, uint32_t count);
int sots_read_select_splitters(sots_ctx *ctx, uint64_t *keys, uint32_t count);
/* List mode of the SPLITTERS selection, for tests: files the key of every row of the current half under its bucket
 * between the splitters the next sots_stage_select reads - what the fused loop's spectral kernel does as it computes the
 * fitness - so that this sots_stage_select takes its buckets from the lists.  Anything that replaces rows, fitness,
 * splitters, target, plan or sort mode in between drops the lists again.  SOTS_ERR_STATE where a slot holds more than
 * 256 splitters, or with SOTS_SELECT_LISTS=0 in the environment of sots_create (the selection then always streams).
 * Like every sots_stage_* it looks at all P rows: rows a lazy selection has left out are produced first (under
 * SOTS_SORT_TOP_ONLY they are not, and what is filed for them is as unspecified as they are). */
int sots_stage_bucket_fitness(sots_ctx *ctx);
/* What sots_stage_bucket_fitness filed, for tests of the filing itself (SOTS_ERR_STATE unless it was the last thing to
 * touch the lists).  With B = sots_select_splitter_count: counts[B * 16] - counter s of bucket j at j * 16 + s, every key
 * of a closed bucket j < B - 1 counted, also those its segment had no place for; the open bucket B - 1 counts nothing -
 * and keys[B * 2048]: segment s of bucket j from (j * 16 + s) * 128 on, min(count, 128) keys in the order they arrived. */
int sots_read_select_lists(sots_ctx *ctx, uint32_t *counts, uint32_t counts_len, uint64_t *keys, uint32_t keys_len);
/* enum sots_synth_arith; applies to sots_stage_synthesise and to both generation loops from the next call on
 * (replaces nothing: the reference picks its arithmetic by picking a backend, main.cpp:105-163) */
int sots_set_synth_arithmetic(sots_ctx *ctx, uint32_t arith);
/* Elitist survival (new; replaces nothing: the reference's strategy keeps no row, ocl_program.cl:99-190).  With n > 0 the
 * variation that makes the new half - sots_stage_recombine + sots_stage_mutate, and the variation of both generation
 * loops, whichever kernel performs it - does this for row i:
 *   i <  n : values and steps are bit copies of row i of the sorted current half; nothing is drawn, nothing is mutated;
 *   i >= n : exactly what is computed with n = 0 (the PRNG is counter-based: the survivors' draws are left out, nobody
 *            else's change).
 * Everything after variation is unchanged: survivors are synthesised and evaluated again like any other row - no fitness
 * is carried that a new target could make stale - and compete in the sort, at a lower row index than any offspring of
 * equal fitness.  n = numParents is plus-selection.  0 <= n <= numParents (rows every sort mode and both selection plans
 * place every generation); above that SOTS_ERR_INVALID, and the old setting stays.  Default 0: the launches and bits of
 * the reference's strategy.  A setting, not population state: sots_init_population, sots_set_target_* and
 * sots_write_population keep it; it applies from the next variation on and neither completes nor drops a pending
 * lazy tail (enum sots_sort_mode).  The rows carried are whatever rows 0..n-1 of the current half hold when variation
 * runs, immigrants of a fused or separate inject included.  Islands of a group are set through sots_group_island. */
int sots_set_survivors(sots_ctx *ctx, uint32_t n);
int sots_get_survivors(const sots_ctx *ctx, uint32_t *n);
/* The spectral objective (new; replaces nothing: the reference has the one fitness, Evolutionary_Strategy.hpp:517-519 /
 * ocl_program.cl:608-611).  With m_k = |X_k| / N / windowFactor, the candidate's normalised magnitude of bin k, and t_k
 * the target's, over the bins k = 0 .. N/2-1 of the reference's sum:
 *   SOTS_OBJECTIVE_MAGNITUDE      F = sum_k (m_k - t_k)^2                            (the reference's; the default)
 *   SOTS_OBJECTIVE_LOG_MAGNITUDE  F = sum_k (ln(m_k + floor) - ln(t_k + floor))^2
 * floor, in the unit of the normalised magnitudes, must be finite with 1e-30 <= floor <= 1 (m + floor is then a normal
 * fp32 number); it is ignored for MAGNITUDE and reported as 0.  An unknown objective or a floor outside the range is
 * SOTS_ERR_INVALID, and the old setting stays.  Setting the objective - to any value, the current one included - acts
 * like a new target: the run record is cleared, the stored splitters and key lists are dropped.  It may come before or
 * after the target, with the same result; sots_read_synth still returns the raw target magnitudes.  NaN rows
 * get NaN fitness and sort last, as ever.  Fitness values, history records and stop-rule thresholds
 * (sots_stop_rule.target_fitness) are in the units of the active objective: squared nepers summed over the bins under
 * LOG_MAGNITUDE.  A setting: sots_init_population and sots_set_target_* keep it. */
enum sots_objective { SOTS_OBJECTIVE_MAGNITUDE = 0, SOTS_OBJECTIVE_LOG_MAGNITUDE = 1 };
int sots_set_objective(sots_ctx *ctx, uint32_t objective, float floor);
int sots_get_objective(const sots_ctx *ctx, uint32_t *objective, float *floor);
/* Per-bin weights of the objective (new; the reference weighs every bin alike, ocl_program.cl:608-611).  With weights
 * w_k, k = 0 .. N/2-1, the fitness under either objective is F = sum_k (u_k e_k)^2 = sum_k w_k e_k^2, where e_k is the
 * bin's signed error as the active objective computes it (m_k - t_k, or ln(m_k + floor) - ln(t_k + floor)) and
 * u_k = sqrtf(w_k), made once.  A weight of 1 leaves the bin's contribution as it is without weights, bit for bit; a weight
 * of 0 makes a finite bin contribute exactly 0.  num_bins must be N/2, every w_k finite and >= 0, at least one > 0:
 * anything else is SOTS_ERR_INVALID and the old setting stays.  NULL with 0 bins removes the weights (the default).
 * Setting or removing them acts like a new target, as sots_set_objective does: the run record is cleared, the stored
 * splitters and key lists are dropped.  Before or after the target and the objective, with the same result;
 * sots_read_synth still returns the raw target magnitudes.  Fitness values, history records and stop-rule thresholds
 * (sots_stop_rule.target_fitness) are in the units of the WEIGHTED sum.  A setting: sots_init_population, sots_set_target_*
 * and sots_set_objective keep it.
 * sots_get_objective_weights: *is_set (may be NULL) says whether weights are set; weights (may be NULL; otherwise
 * num_bins must be N/2) receives the w_k as they were passed, and is left alone when none are set. */
int sots_set_objective_weights(sots_ctx *ctx, const float *weights, uint32_t num_bins);
int sots_get_objective_weights(const sots_ctx *ctx, float *weights, uint32_t num_bins, uint32_t *is_set);
int sots_get_generation(const sots_ctx *ctx, uint32_t *generation);
int sots_set_generation(sots_ctx *ctx, uint32_t generation);

/* ---- overlap-add rendering of a parameter track (new; the reference writes the last chunk's best row and stops,
 *      main.cpp:270-275) ----
 * values is [num_rows][D] unit-range genes, as sots_write_population takes them; row c is the individual that stands for
 * samples [c hop, c hop + N) of the output.  With a_c row c's audio as sots_stage_synthesise makes it under the context's
 * voice and sots_set_synth_arithmetic mode, and w the context's fp32 window table (1 - cos, periodic: w[0] = 0, peak 2) or
 * all ones without SOTS_RENDER_WINDOWED,
 *   acc[n] = sum w[n - c hop] * a_c[n - c hop]   over the chunks c that cover n, in ASCENDING c,
 *   den[n] = sum w[n - c hop]                    the same chunks, the same order,
 *   out[n] = den[n] > 0 ? acc[n] / den[n] : 0    (samples no chunk covers are 0: n >= (num_rows - 1) hop + N)
 * all in fp32: one multiply and one add per term, uncontracted, and the correctly rounded division - the same inputs give
 * the same bits on every run (a gather: no atomics), tests/_render_model.py states them in NumPy.  Rectangular with
 * hop = N the output is the rows' audio end to end.
 * The work goes in passes: a pass produces the samples of rows_per_pass consecutive chunk starts and synthesises, into
 * render scratch of the context's own (allocated by the first call, freed with the context), those chunks and the
 * ceil(N / hop) - 1 chunks in front of them that reach into its range - chunks that straddle a pass boundary are
 * synthesised again.  The result does not depend on the pass size.  out (host memory) receives out_samples samples:
 * fewer than the covered range truncates, more gives zeros.
 * Blocking.  The population, both rotation halves, the audio and spectrum buffers, fitness, generation counter, run
 * record, splitters and lists are untouched.  SOTS_ERR_INVALID for null or mis-sized args, a hop outside
 * ceil(N / 64) .. N, unknown flag bits or num_rows == 0; SOTS_ERR_SIZE for values_bytes != num_rows * D * 4. */
enum sots_render_flags { SOTS_RENDER_WINDOWED = 1 };
typedef struct sots_render_args {
    uint32_t struct_size;    /* = sizeof(sots_render_args) */
    uint32_t hop;            /* samples between chunk starts, ceil(N/64) <= hop <= N, need not divide N */
    uint32_t flags;          /* enum sots_render_flags */
    uint32_t rows_per_pass;  /* 0 = the library's choice; else chunk starts per pass, >= 1 */
} sots_render_args;
int sots_render_overlap_add(sots_ctx *ctx, const float *values, size_t values_bytes, uint32_t num_rows,
                            const sots_render_args *args, float *out, uint64_t out_samples);

/* ---- phase-continuous rendering of a parameter track (new) ----
 * The overlap-add rendering starts every row at phase 0, so overlapping rows of one stationary tone are 2 pi f hop / sr out
 * of phase and their weighted mean is a comb filter in f.  This renders the track as ONE voice whose oscillators never
 * restart.  Inputs as sots_render_overlap_add: values [num_rows][D] unit-range genes, 1 <= hop <= N, the context's voice,
 * param_min / param_max and wavetable tab; S = (num_rows - 1) hop + N output samples.
 * Row position of sample n: row c is anchored at the centre of the samples it analysed, c hop + N/2.  m = n - N/2; for
 *   m <= 0: k = 0, r = 0; otherwise k = m / hop, r = m % hop; for k >= num_rows - 1: k = num_rows - 1, r = 0.
 * Genes at n: HOLD (the default) row k + (2 r >= hop ? 1 : 0) as it is.  SOTS_RENDER_GLIDE: for r = 0 row k as it is,
 *   otherwise t = (float)r / (float)hop (correctly rounded) and g_d = v[k][d] + t * (v[k+1][d] - v[k][d]) in fp32:
 *   subtract, multiply, add, uncontracted.
 * Parameters and derived products at n: the fp32 expressions of the reference's CPU path (Evolutionary_Strategy.hpp:368-495),
 *   per sample: p = min + g (max - min) (the triple voice scales by entries d & 3), m1 = p0 p1, inc1 = c p0 or c p1, ...,
 *   c = 32768 / 44100.0f.
 * Phases: unsigned 15.17 fixed point in 32-bit words, so the wrap at W = 32768 is the wrap of the word.
 *   fix(x): y = x * 131072.0f; rint(y), ties to even, reduced mod 2^32 (a negative increment is its two's complement);
 *   0 where |y| < 2^62 does not hold.  Every operator: Phi(0) = 0, Phi(n+1) = Phi(n) + fix(inc(n)) mod 2^32, and its table
 *   read is tab[Phi(n) >> 17]: always in range, no clamp, no wrap tests.  inc(n) of the first operator is the
 *   constant-frequency increment; of a later one c cur(n) with cur(n) = tab[Phi_prev(n) >> 17] m + off as the reference
 *   writes it, Phi_prev(n) being the operator before it BEFORE that operator's update.
 * Output: tab[Phi_last(n) >> 17] amp, the reference's last line per voice; the triple voice: the three chains' products
 *   added in order and divided by 3 as the synthesis kernels do.  Samples at n >= S are +0; a shorter out_samples truncates.
 * An operator's phase is thus the exclusive prefix sum of its increments, and integer addition is associative: the bits do
 * not depend on tiles, grids or passes, and tests/_render_continuous_model.py (NumPy, cumsum in uint32) is exact.  For
 * one row the output is that row's voice, close to but not bit for bit sots_stage_synthesise's: the phase has 17
 * fractional bits where fp32 has 8 near W.
 * The work goes in passes of samples_per_pass output samples; a pass starts from the end phases of the pass before it (one
 * word per operator: all the state there is).  Render scratch of the context's own as above.  Blocking; population, audio,
 * spectrum, fitness, generation counter, run record, splitters and lists are untouched.
 * SOTS_ERR_INVALID for null or mis-sized args, a hop outside 1 .. N, unknown flag bits, num_rows == 0 or S >= 2^31;
 * SOTS_ERR_SIZE for values_bytes != num_rows * D * 4; SOTS_ERR_STATE under SOTS_ARITH_DEVICE_KERNELS (that mode exists to be
 * the reference's device kernels bit for bit, and its 3-op voice reads another offset). */
enum sots_render_continuous_flags { SOTS_RENDER_GLIDE = 1 };
typedef struct sots_render_continuous_args {
    uint32_t struct_size;      /* = sizeof(sots_render_continuous_args) */
    uint32_t hop;              /* samples between row anchors, 1 <= hop <= N */
    uint32_t flags;            /* enum sots_render_continuous_flags */
    uint32_t samples_per_pass; /* 0 = the library's choice; else output samples per pass, >= 1 */
} sots_render_continuous_args;
int sots_render_continuous(sots_ctx *ctx, const float *values, size_t values_bytes, uint32_t num_rows,
                           const sots_render_continuous_args *args, float *out, uint64_t out_samples);

/* ---- phase-continuous rendering of a parameter track of the operator-graph voice (new) ----
 * sots_render_continuous for a context of sots_create_graph: the track as ONE graph voice whose oscillators never restart.
 * Inputs, row position of sample n, HOLD / SOTS_RENDER_GLIDE, fix(), S = (num_rows - 1) hop + N and "+0 at n >= S" are those
 * of sots_render_continuous; sots_render_continuous_args and its flags are reused.  The graph, its waveform codes w_j and
 * param_min / param_max are the context's.
 * Genes at n are scaled as the graph voice scales them: p_g = pmin_g + g_g (pmax_g - pmin_g), no `& 3` folding, D = 2 OPS.
 *   f_j = p(2j), a_j = p(2j+1); A_j = f_j a_j for a modulator, a_j for a carrier; c = (float)W / 44100.
 * Operators in ascending j, all fp32 and uncontracted:
 *   Phi_j(0) = 0.
 *   t_j(n)   = shape(w_j, Phi_j(n) >> 17), o_j(n) = t_j(n) A_j(n).  shape is the table of sots_set_voice_waveforms, on the
 *              integer index; the index is always in range, so there is no clamp.  The product is always formed.
 *   cur_j(n) = f_j for an unmodulated operator, otherwise ((o_i1 + o_i2) + ...) + f_j over the set bits of modulators[j] in
 *              ascending i: the sum starts from the first term, and a clear bit is skipped, not added as 0.
 *   Phi_j(n+1) = Phi_j(n) + fix(c cur_j(n)) mod 2^32.  A non-finite or huge cur gives an increment of 0, as fix says.  There
 *              is no wrap test and no lower-wrap distinction between modulated and unmodulated operators: the word wraps.
 *   out[n]   = ((o_c1 + o_c2) + ...) over the carriers in ascending j, divided by (float)count, correctly rounded, where
 *              there is more than one.
 * Every operator's phase is the exclusive prefix sum of its increments, so the bits do not depend on tiles, grids or passes;
 * tests/_render_graph_continuous_model.py (NumPy, cumsum in uint32) is exact.
 * Anchors, both bit for bit: the graph {0->1, carrier 1} is sots_render_continuous of SOTS_SYNTH_2OP, and {0->1, 2->3, 4->5,
 * carriers 1, 3, 5} with the ranges of genes 0..3 repeated per pair is that of SOTS_SYNTH_TRIPLE_PAR.
 * Feedback is not rendered: with beta_j != 0, t_j(n) depends on t_j(n-1) and t_j(n-2) through a table lookup, a serial,
 * non-associative recurrence over the whole rendering that no scan computes.  A context with any beta_j != 0 is refused;
 * sots_render_overlap_add renders such a voice.
 *
 *   renderer                       voices                                  a row's phase          overlapping rows
 *   sots_render_overlap_add        all five, waveforms, feedback           restarts at 0          window-weighted mean (a comb)
 *   sots_render_continuous         the four fixed voices                   carried, 15.17 words   one voice
 *   sots_render_graph_continuous   the graph voice, waveforms, no feedback carried, 15.17 words   one voice
 *   sots_render_graph_feedback     the graph voice, waveforms, feedback    carried, words + h1 h2 one voice
 *   sots_render_graph_genes        ... and feedback indices that are genes carried, words + h1 h2 one voice, beta per sample
 *
 * The work goes in passes of samples_per_pass output samples (0: the library's choice, the most that keeps the phase words
 * of a pass, one per operator and sample, within 96 MiB: 2^22 samples up to 6 operators, 3 592 192 for 7, 3 145 728 for 8);
 * a pass starts from the end phases of the pass before it, one word per operator: all the state there is.  Render scratch of
 * the context's own as above.  Blocking; population, audio, spectrum, fitness, generation counter, run record, splitters and
 * lists are untouched.
 * SOTS_ERR_STATE for a context of a fixed voice and for a context with a feedback index != 0 (the text names
 * sots_set_voice_feedback); SOTS_ERR_INVALID for null or mis-sized args, a hop outside 1 .. N, unknown flag bits,
 * num_rows == 0, S >= 2^31 or a null out with out_samples > 0; SOTS_ERR_SIZE for values_bytes != num_rows * D * 4. */
int sots_render_graph_continuous(sots_ctx *ctx, const float *values, size_t values_bytes, uint32_t num_rows,
                                 const sots_render_continuous_args *args, float *out, uint64_t out_samples);

/* ---- ... with feedback operators (new) ----
 * sots_render_graph_continuous for a context whose operators may have a feedback index beta_j (sots_set_voice_feedback).
 * Everything of sots_render_graph_continuous holds unchanged: inputs, row position, HOLD / SOTS_RENDER_GLIDE, fix(),
 * S = (num_rows - 1) hop + N and +0 at n >= S, gene scaling, A_j, c, cur_j, Phi_j(n+1) = Phi_j(n) + fix(c cur_j(n)) mod 2^32,
 * the carrier sum and its division.  Feedback never changes Phi_j: every phase is still the exclusive prefix sum of its
 * increments.  What differs is t_j(n) of an operator with beta_j != 0.
 *   beta_j == 0:  t_j(n) = shape(w_j, Phi_j(n) >> 17), as above.
 *   beta_j != 0:  h1_j = h2_j = +0 at sample 0 of the rendering, and per sample, all fp32 and uncontracted:
 *       K   = 0x1.45f306p+12f            (the constant of sots_set_voice_feedback)
 *       B_j = beta_j * K                 (one product)
 *       g   = (h1_j + h2_j) * 0.5f
 *       z   = Phi_j(n) + fix(B_j * g)  mod 2^32     (the word wraps: no wrap tests, no clamp)
 *       t_j(n) = shape(w_j, z >> 17);  o_j(n) = t_j(n) * A_j(n)
 *       h2_j = h1_j;  h1_j = t_j(n)
 *     h is the shaped value before the level, so |h| <= 1 and |B_j g| <= 2 K < W: the offset is always finite and fix never
 *     takes its zero branch.  A modulator's o_i(n), as the operators it modulates and the mix read it, is made from t_i(n).
 * With every beta zero the call is sots_render_graph_continuous bit for bit (the same launches).  For one row the output is
 * that row's voice, close to but not bit for bit sots_stage_synthesise's, as above.
 * t_j(n) depends on t_j(n-1) and t_j(n-2) through a table lookup: a chain over the samples that no scan computes.  The chain
 * has exactly one solution, since the carry into it is given and every sample is a function of the two before it; however
 * it is computed (chain_form), the output is that solution, and the bits do not depend on chain_form, relax_cap, tiles,
 * grids or passes.  tests/_render_graph_feedback_model.py states it twice in NumPy, as a loop and as a relaxation.
 *   chain_form 1  serial: one wavefront per feedback operator walks the samples in order.
 *   chain_form 2  relaxation: per tile of 1024 samples, start from the feed-forward values and recompute every sample from
 *                 its two predecessors in the previous sweep, all samples at once, until a sweep changes no bit (sweep k makes
 *                 at least the first k samples final); after relax_cap sweeps the tile is finished serially from sample
 *                 relax_cap on.
 *   chain_form 0  the library's choice per operator, a rule on beta_j (csrc/sots_rules.h): the relaxation for beta_j <= 1.5,
 *                 where it was measured to be faster, the serial form above; relax_cap 0 is 1024.
 * Passes as above; with FB feedback operators a pass holds at most floor(96 MiB / (4 (OPS + FB)) / 4096) tiles of 4096
 * samples, and at most 1024 tiles; a pass starts from the end phases of the pass before it and from h1_j, h2_j of every
 * feedback operator.  Blocking; everything else of the context is untouched.
 * SOTS_ERR_STATE for a context of a fixed voice; SOTS_ERR_INVALID for null or mis-sized args, a hop outside 1 .. N, unknown
 * flag bits, chain_form > 2, relax_cap > 4096, num_rows == 0, S >= 2^31 or a null out with out_samples > 0; SOTS_ERR_SIZE for
 * values_bytes != num_rows * D * 4. */
typedef struct sots_render_graph_feedback_args {
    uint32_t struct_size;      /* = sizeof(sots_render_graph_feedback_args) */
    uint32_t hop;              /* as sots_render_continuous_args */
    uint32_t flags;            /* enum sots_render_continuous_flags */
    uint32_t samples_per_pass; /* 0 = the library's choice; else output samples per pass, >= 1 */
    uint32_t chain_form;       /* 0 = the library's choice, 1 = serial, 2 = relaxation */
    uint32_t relax_cap;        /* sweeps per tile before a tile is finished serially; 0 = the library's choice, else 1..4096 */
} sots_render_graph_feedback_args;
int sots_render_graph_feedback(sots_ctx *ctx, const float *values, size_t values_bytes, uint32_t num_rows,
                               const sots_render_graph_feedback_args *args, float *out, uint64_t out_samples);

/* ---- ... whose feedback indices are genes (new) ----
 * sots_render_graph_feedback for a context of sots_create_graph_genes: a track as the matcher writes it for that voice,
 * rendered as ONE voice whose oscillators never restart and whose feedback index follows the rows.  The args struct and its
 * flags are those of sots_render_graph_feedback, and everything of that call holds: inputs, row position of sample n, HOLD /
 * SOTS_RENDER_GLIDE, fix(), S and +0 at n >= S, gene scaling, A_j, c, cur_j, the phase recurrence, the carrier sum and its
 * division, h1 = h2 = +0 at sample 0, chain_form and relax_cap, passes and what a pass carries.  What differs:
 *   Row width.  values is [num_rows][D] with D = 2 OPS + E, the context's D.  Genes 0 .. 2 OPS - 1 mean what they mean in
 *     every graph voice; gene 2 OPS + r is the index of the operator with the r-th set bit of the mask, ascending.
 *   The index at sample n.  For an operator j of the mask, with q its gene column:
 *       g_q(n)  the raw gene at n: the row's (HOLD) or v_k + t (v_k+1 - v_k) (GLIDE), as any gene
 *       p(n)    = pmin_q + g_q(n) (pmax_q - pmin_q)
 *       beta_j(n) = p(n) > 0 ? fminf(p(n), 2) : +0     (NaN, negative values and -0 give +0; values above 2 give 2)
 *       B_j(n)  = beta_j(n) * K                        (one fp32 product, uncontracted)
 *     and the chain step at n uses B_j(n): z = Phi_j(n) + fix(B_j(n) * g) mod 2^32.  Nothing else changes.
 *   A gene operator ALWAYS runs the chain, as in the voice itself, also where beta_j(n) = +0.  In the rendering that cannot be
 *     seen in the bits: fix(+0 * g) = 0 for every g (|g| <= 1), so z = Phi_j(n), the word wraps and is never clamped, and
 *     t_j(n) = shape(w_j, Phi_j(n) >> 17), the feed-forward value.
 *   The other operators keep the context's index (sots_set_voice_feedback); those with beta_j != 0 run the chain with their
 *     constant B_j as in sots_render_graph_feedback.  The operators that run a chain ("flagged") are the mask's and these.
 * Anchors, both bit for bit.  (a) On a context whose mask is 0 the call is sots_render_graph_feedback: the same launches with
 * the same arguments.  (b) A track whose effective index is the constant b_j on every gene operator (a gene range [b_j, b_j]
 * and any finite gene value, HOLD or GLIDE) renders to what sots_render_graph_feedback gives for a context of
 * sots_create_graph with the same graph, waveforms and ranges and sots_set_voice_feedback = b_j on those operators, fed the
 * same rows without their gene columns; b_j anywhere in [0, 2], 0 included.
 * The chain has one solution whether B is one constant or a value per sample: the carry into it is given and every sample is
 * a function of the two before it and of its own B.  The bits do not depend on chain_form, relax_cap, tiles, grids or passes;
 * tests/_render_graph_genes_model.py states it in NumPy, the chain twice.
 *   chain_form 0  the library's choice per operator: an operator of the mask is relaxed, whatever its rows hold (at every
 *                 index up to 1.5 the relaxation was measured faster, and at 2 it cost what the serial form costs; nothing in
 *                 between was measured); every other flagged operator by the rule of sots_render_graph_feedback.
 * A pass holds what it holds there, with the flagged operators counted as FB.
 * SOTS_ERR_STATE for a context of a fixed voice; SOTS_ERR_INVALID and SOTS_ERR_SIZE as sots_render_graph_feedback, under this
 * call's name, with D the context's: values_bytes != num_rows * D * 4 is SOTS_ERR_SIZE. */
int sots_render_graph_genes(sots_ctx *ctx, const float *values, size_t values_bytes, uint32_t num_rows,
                            const sots_render_graph_feedback_args *args, float *out, uint64_t out_samples);

/* ---- per-stage device timing (feeds Benchmarker::addTimer, Benchmarker.hpp:109-130) ---- */
int sots_timing_enable(sots_ctx *ctx, int enabled);
int sots_timing_reset(sots_ctx *ctx);
/* sum of hipEvent-measured durations and the number of launches of that stage
 * since the last reset; synchronises the stream */
int sots_stage_time_ms(sots_ctx *ctx, int stage, double *total_ms, uint64_t *count);
/* the individual launch durations behind that sum, oldest first (at most 65536 are kept per stage
 * between resets): one Benchmarker::addTimer(name, ms) per launch gives the CSV the reference's
 * per-launch Average/Max/Min columns (Benchmarker.hpp:33-72,109-130).  *written <= capacity. */
int sots_stage_launch_times_ms(sots_ctx *ctx, int stage, float *out_ms, uint64_t capacity, uint64_t *written);

/* ---- island model (new) ----
 * A row is [fitness, v0..v(D-1), s0..s(D-1)] = (2D+1) floats.  pack copies the best
 * n_rows rows of the current (sorted) half; inject overwrites the last n_rows of the
 * PARENT rows that recombination reads - whole blocks of workgroupSize rows:
 * B = max(1, numParents / workgroupSize) * workgroupSize, rows B-n_rows .. B-1
 * (= numParents-n_rows .. numParents-1 when numParents is a multiple of the block,
 * ocl_program.cl:99-112) - so that immigrants take part in the next recombination.  *_device take device pointers on this context's
 * device and run on its stream (no host sync); *_host are blocking. */
int sots_pack_elites_device(sots_ctx *ctx, void *device_rows, uint32_t n_rows);
int sots_inject_immigrants_device(sots_ctx *ctx, const void *device_rows, uint32_t n_rows);
/* gathered_rows = the all-gather result, world x elites rows in rank order: injects every
 * island's rows except this rank's own block (one launch, no intermediate copy) */
int sots_inject_gathered_device(sots_ctx *ctx, const void *gathered_rows, uint32_t world, uint32_t rank,
                                uint32_t elites);
/* The same exchange WITHOUT its two launches: the sortPopulation of the LAST generation of the next
 * sots_execute_generations call also (a) takes the immigrant rows straight from gathered_rows (as
 * sots_inject_gathered_device would after that sort) and (b) writes the best n_elite_rows rows of the result, immigrants
 * included where the ranges overlap, to elite_rows (as sots_pack_elites_device would after the inject).  Either
 * pointer may be NULL; both are device pointers that must be ready when that sort runs on the context's stream and
 * stay valid until it has.  Used once, then forgotten; sots_init_population forgets it too.  Where sortPopulation
 * places only the rows recombination reads (enum sots_sort_mode), n_elite_rows may not exceed them.
 * host_gate_event (optional, a hipEvent_t): for gathered_rows filled by a collective on ANOTHER stream.  The host waits
 * for the event (hipEventSynchronize) right before it enqueues that sort - the generation's variation, synthesis and
 * spectral kernels are on the stream by then, so the device stays busy - instead of the stream waiting for it: on this
 * runtime a cross-stream hipStreamWaitEvent costs the waiting stream ~18 us per generation even for an event that
 * completed long ago.  With NULL the caller orders the rows on the context's stream itself. */
int sots_fuse_exchange_next_sort(sots_ctx *ctx, void *elite_rows, uint32_t n_elite_rows, const void *gathered_rows,
                                 uint32_t world, uint32_t rank, uint32_t elites, void *host_gate_event);
int sots_pack_elites_host(sots_ctx *ctx, float *rows, uint32_t n_rows);
int sots_inject_immigrants_host(sots_ctx *ctx, const float *rows, uint32_t n_rows);

/* ---- island group: one process, one island per listed device (new) ----
 * The reference has one device per process (Evolutionary_Strategy_OpenCL.hpp:194-226).  A group owns one
 * sots_ctx per entry of `devices` (island i: device devices[i], PRNG ids gid_base + i * P, so an island's
 * random stream does not depend on the group size) and runs them from one host thread each.  Every
 * `migration_interval` generations each island's best `num_elites` rows are all-gathered - RCCL
 * (ncclCommInitAll + ncclAllGather on the islands' streams, librccl opened on first use) when the devices
 * are distinct, device-to-device copies ordered by HIP events when islands share a device - and the other
 * islands' rows overwrite the tail of the rows recombination reads (sots_inject_gathered_device).
 * With one device the group is that one island and exchanges nothing. */
#define SOTS_MAX_GROUP_DEVICES 16
enum sots_group_flags {
    SOTS_GROUP_OVERLAP = 1,    /* the all-gather started after generation g runs on a side stream underneath
                                * generation g+1 and is injected after g+1's sort (rows arrive one exchange later) */
    SOTS_GROUP_FORCE_RCCL = 2, /* use RCCL even for a single island (a one-rank communicator; exercises the
                                * collective path on a one-GPU machine) */
    SOTS_GROUP_EVENT_WAITS = 8,/* overlapped schedule: the island's STREAM waits for the side stream's events instead of its host
                                * thread (sots_fuse_exchange_next_sort, host_gate_event): same results, ~18 us per
                                * generation slower on this runtime; for tests and timing comparisons */
    SOTS_GROUP_UNFUSED = 4     /* pack and inject as launches of their own (sots_pack_elites_device,
                                * sots_inject_gathered_device) instead of inside the sort kernels
                                * (sots_fuse_exchange_next_sort): same results, for tests and timing comparisons */
};
typedef struct sots_group sots_group;
int sots_group_create(const sots_config *island_cfg, const int32_t *devices, uint32_t num_devices,
                      uint32_t num_elites, uint32_t migration_interval, uint32_t flags, sots_group **out);
void sots_group_destroy(sots_group *group);
/* text of the last failure on the group (or of the last failed sots_group_create when group == NULL) */
const char *sots_group_last_error(const sots_group *group);
uint32_t sots_group_size(const sots_group *group);
int sots_group_uses_rccl(const sots_group *group);
/* island i's context: read its population, timers, info; do not destroy it or change its stream */
sots_ctx *sots_group_island(sots_group *group, uint32_t i);
int sots_group_set_target_audio(sots_group *group, const float *audio, uint32_t num_samples);
int sots_group_set_target_spectrum(sots_group *group, const float *magnitudes, uint32_t num_bins);
/* sots_set_objective on every island (new; the reference has one fitness, ocl_program.cl:608-611); the first failure is returned */
int sots_group_set_objective(sots_group *group, uint32_t objective, float floor);
/* sots_set_objective_weights on every island (new); the first failure is returned */
int sots_group_set_objective_weights(sots_group *group, const float *weights, uint32_t num_bins);
int sots_group_init_population(sots_group *group, uint32_t chunk_index);
/* n generations on every island with the elite exchange; returns once everything is ENQUEUED.  In the overlapped
 * schedule (SOTS_GROUP_OVERLAP without SOTS_GROUP_EVENT_WAITS, "host-gated") every island's thread waits, before it
 * enqueues the sort of a generation in which an exchange falls due, for the PREVIOUS exchange's all-gather to have
 * completed on the device: the call can block for up to that long, and the host runs at most one exchange interval
 * ahead of the devices.  This schedule over RCCL has run on a one-rank communicator only (no machine with two GPUs has
 * been available to the tests); SOTS_GROUP_EVENT_WAITS is the stream-ordered fallback.
 * After an error the islands' populations are unspecified (a failed island stops running generations, the others go on
 * and may receive its last good - or +inf-fitness - rows). */
int sots_group_execute_generations(sots_group *group, uint32_t n);
int sots_group_synchronize(sots_group *group);
/* the island holding the lowest fitness and that fitness (blocking) */
int sots_group_best(sots_group *group, uint32_t *island, float *fitness);

/* ---- chunks in flight (new; the reference's parameterMatchAudio, Evolutionary_Strategy_OpenCL.hpp:572-610) ----
 * One handle advances up to max_chunks independent populations, each of the shape cfg describes and each against
 * its own target, with the launches of ONE population per generation (recombine+mutate | synthesise |
 * window+FFT+fitness | sort, each over every active chunk's rows).  Chunk c of the batch computes bit for bit what a
 * sots_ctx of the same cfg computes after sots_init_population(ctx, first_chunk_index + c) and the same calls.
 * Limits: populationLength <= 1024 per chunk, max_chunks >= 1, max_chunks * populationLength <= 2^26.  Every
 * generation sorts all rows of every chunk (SOTS_SORT_FULL; at these sizes a context does too).
 * Rows are chunk-major: chunk c holds rows [c P, (c+1) P) of each rotation half. */
typedef struct sots_batch sots_batch;
int sots_batch_create(const sots_config *cfg, uint32_t max_chunks, sots_batch **out);
/* chunks of the operator-graph voice (sots_create_graph above: the same rules for cfg and graph) */
int sots_batch_create_graph(const sots_config *cfg, const sots_voice_graph *graph, uint32_t max_chunks, sots_batch **out);
void sots_batch_destroy(sots_batch *b);
/* text of the last failure on b (or of the last failed sots_batch_create when b == NULL) */
const char *sots_batch_last_error(const sots_batch *b);
int sots_batch_synchronize(sots_batch *b);
/* num_chunks (1..max_chunks) targets: chunk c = samples [c N, (c+1) N) / bins [c N/2, (c+1) N/2).  num_samples >=
 * num_chunks * N; num_bins == num_chunks * N/2.  Sets the number of ACTIVE chunks for the calls below. */
int sots_batch_set_target_audio(sots_batch *b, const float *audio, uint32_t num_samples, uint32_t num_chunks);
int sots_batch_set_target_spectra(sots_batch *b, const float *magnitudes, uint32_t num_bins, uint32_t num_chunks);
/* the audio form with chunk k = samples [k hop, k hop + N), 1 <= hop <= N (SOTS_ERR_INVALID otherwise): analysis at a hop.
 * num_samples >= (num_chunks - 1) hop + N, else SOTS_ERR_SIZE.  sots_batch_set_target_audio is the hop = N case of the
 * same code. */
int sots_batch_set_target_audio_hop(sots_batch *b, const float *audio, uint32_t num_samples, uint32_t hop, uint32_t num_chunks);
/* active chunk c is initialised exactly as sots_init_population(ctx, first_chunk_index + c) would */
int sots_batch_init_population(sots_batch *b, uint32_t first_chunk_index);
/* n generations of every active chunk; only enqueues */
int sots_batch_execute_generations(sots_batch *b, uint32_t n);
int sots_batch_set_synth_arithmetic(sots_batch *b, uint32_t arith); /* enum sots_synth_arith */
/* sots_set_survivors for every chunk of the batch, in sots_batch_execute_* and sots_batch_queue_run alike (a refilled
 * slot's first variation carries the initialised rows 0..n-1, as a fresh context's does); same limits, same default */
int sots_batch_set_survivors(sots_batch *b, uint32_t n);
/* sots_set_objective for every chunk of the batch (new; the reference has one fitness, ocl_program.cl:608-611), in
 * sots_batch_execute_* and sots_batch_queue_run alike: the active targets' and the stored queue targets' tables are
 * rebuilt for it, every chunk's run record is cleared.  Before or after the targets, with the same result. */
int sots_batch_set_objective(sots_batch *b, uint32_t objective, float floor);
/* sots_set_objective_weights for every chunk of the batch (new), in sots_batch_execute_* and sots_batch_queue_run alike:
 * one table for all chunks, active and queued.  Every chunk's run record is cleared.  Before or after the targets and
 * the objective, with the same result. */
int sots_batch_set_objective_weights(sots_batch *b, const float *weights, uint32_t num_bins);
/* sots_set_voice_waveforms for every chunk of a graph-voice batch (new), in sots_batch_execute_* and
 * sots_batch_queue_run alike: one setting for all chunks, the same rules and refusals.  Every chunk's run record is
 * cleared.  Before or after the targets, the objective and the weights, with the same result. */
int sots_batch_set_voice_waveforms(sots_batch *b, const uint32_t *codes, uint32_t count);
int sots_batch_get_voice_waveforms(const sots_batch *b, uint32_t codes[8]);
/* sots_set_voice_feedback for every chunk of a graph-voice batch (new): one setting for all chunks, the same rules and
 * refusals.  Every chunk's run record is cleared.  In any order with the targets, objective, weights and waveforms. */
int sots_batch_set_voice_feedback(sots_batch *b, const float *index, uint32_t count);
int sots_batch_get_voice_feedback(const sots_batch *b, float index[8]);
/* sots_create_graph_genes for a batch (new): every chunk's individuals carry the feedback indices of the masked operators */
int sots_batch_create_graph_genes(const sots_config *cfg, const sots_voice_graph *graph, uint32_t feedback_genes, uint32_t max_chunks,
                                  sots_batch **out);
int sots_batch_get_voice_feedback_genes(const sots_batch *b, uint32_t *feedback_genes);
/* sots_set_graph_synth_form for a graph-voice batch (new), in sots_batch_execute_* and sots_batch_queue_run alike: the same
 * rules and refusals; nothing is cleared.  `effective` is for one launch of all max_chunks x P rows of the batch. */
int sots_batch_set_graph_synth_form(sots_batch *b, uint32_t form);
int sots_batch_get_graph_synth_form(const sots_batch *b, uint32_t *requested, uint32_t *effective);
/* row 0 (the best) of every active chunk: values [active][D], fitness [active] (either may be NULL); blocking */
int sots_batch_read_best(sots_batch *b, float *values, size_t values_bytes, float *fitness, size_t fitness_bytes);
/* one active chunk's current half; byte counts as sots_read_population; blocking */
int sots_batch_read_population(sots_batch *b, uint32_t chunk, float *values, size_t values_bytes,
                               float *steps, size_t steps_bytes, float *fitness, size_t fitness_bytes);

/* ---- run record: best-ever individual, per-generation history, stop rules (new) ----
 * The strategy is not elitist: recombination rewrites every row, the parent blocks included (ocl_program.cl:99-148), and
 * mutation then changes every gene of every row, so row 0 after generation g can be worse than row 0 after g-1 - and
 * the reference's printBest (Evolutionary_Strategy_OpenCL.hpp:612-631) and parameterMatchAudio (:572-610) report row 0 of
 * the LAST generation, after a fixed number of them.  With tracking on, one small kernel after each generation's
 * sortPopulation keeps, on the device and without a host round trip,
 *   - the best individual seen so far (values, steps, fitness, the generation counter when it was seen): a row replaces
 *     the record only when its fitness is strictly lower - a tie keeps the older record, NaN never wins;
 *   - a record of the parent rows 0..numParents-1 whenever the generation counter is a multiple of history_every.
 * It reads the parent rows only (every sort mode places them every generation) and writes nothing the loop reads: the
 * population is bit for bit what it is with tracking off.  The means are pairwise sums in a fixed order, no atomics: the
 * same population gives the same record bits run to run, and a batch chunk gives those of a single context.
 * Both loops record: sots_execute_generations, and sots_execute_generation after its rotate; the single sots_stage_*
 * calls do not.  A record describes the population as the sort left it, immigrants of a fused exchange
 * (sots_fuse_exchange_next_sort) included, rows injected by a later launch not.  Off by default; with tracking off the
 * loops enqueue exactly the launches they always did.  Islands of a group are tracked through sots_group_island. */
typedef struct sots_gen_record {      /* 96 bytes */
    uint32_t generation;              /* generations completed when taken (the context's counter after the sort) */
    float best_fitness;               /* row 0 */
    float best_ever_fitness;          /* after this generation's update */
    float parent_worst_fitness;       /* row numParents-1 */
    float parent_mean_fitness;
    float reserved[3];                /* 0 */
    float mean_step[SOTS_MAX_DIMS];   /* arithmetic mean of steps[0..numParents-1][d]; entries >= D are 0 */
} sots_gen_record;
enum sots_track_flags { SOTS_TRACK_BEST_EVER = 1, SOTS_TRACK_HISTORY = 2 /* implies SOTS_TRACK_BEST_EVER */ };
typedef struct sots_stop_rule {
    uint32_t struct_size;       /* = sizeof(sots_stop_rule) */
    uint32_t check_interval;    /* generations between looks, >= 1 */
    float target_fitness;       /* holds when best-ever fitness <= target; negative = off */
    uint32_t stall_generations; /* holds when generation - best-ever generation >= this (saturating); 0 = off */
} sots_stop_rule;

/* flags 0 frees the buffers and restores the untracked launch sequence; any other call (re)allocates and starts from
 * cleared records.  With SOTS_TRACK_HISTORY history_every and history_capacity must be >= 1: the store is a ring of the
 * newest history_capacity records.  Blocking (synchronises the stream). */
int sots_track(sots_ctx *ctx, uint32_t flags, uint32_t history_every, uint32_t history_capacity);
/* any pointer may be NULL; byte counts must equal D*4.  A cleared record is fitness +inf, generation 0, zeroed rows:
 * sots_init_population and sots_set_target_* clear it (and the history), sots_write_population and
 * sots_set_generation do not.  SOTS_ERR_STATE without SOTS_TRACK_BEST_EVER.  Blocking. */
int sots_read_best_ever(sots_ctx *ctx, float *values, size_t values_bytes, float *steps, size_t steps_bytes,
                        float *fitness, uint32_t *generation);
/* the newest records, oldest first: *written = min(records held, capacity) (the newest of them when capacity is
 * smaller), *taken (may be NULL) = records taken since the last clear.  SOTS_ERR_STATE without SOTS_TRACK_HISTORY.  Blocking. */
int sots_read_history(sots_ctx *ctx, sots_gen_record *out, uint32_t capacity, uint32_t *written, uint64_t *taken);
/* 1 when the rule holds, 0 when not, SOTS_ERR_INVALID for a null rule, a wrong struct_size or check_interval 0.  A rule
 * with both conditions off never holds.  Pure host code: no device, no context. */
int sots_stop_rule_holds(const sots_stop_rule *rule, float best_ever_fitness, uint32_t best_ever_generation,
                         uint32_t generation);
/* sots_execute_generations in blocks of rule->check_interval generations (the last one shorter when max_generations is
 * not a multiple); after each block the best-ever {fitness, generation} come back through a small asynchronous copy to
 * pinned memory and a stream synchronise, and sots_stop_rule_holds decides.  No look-ahead: *generations_run is the first
 * block boundary at which the rule holds, or max_generations.  Needs SOTS_TRACK_BEST_EVER (SOTS_ERR_STATE). */
int sots_execute_until(sots_ctx *ctx, uint32_t max_generations, const sots_stop_rule *rule, uint32_t *generations_run);

/* the same for chunks in flight: every chunk keeps its own record, bit-identical to that of a tracked sots_ctx running
 * chunk first_chunk_index + c.  sots_batch_init_population and sots_batch_set_target_* clear every chunk's record. */
int sots_batch_track(sots_batch *b, uint32_t flags, uint32_t history_every, uint32_t history_capacity);
/* values, steps: [active][D]; fitness, generation: [active]; any pointer may be NULL, byte counts must match */
int sots_batch_read_best_ever(sots_batch *b, float *values, size_t values_bytes, float *steps, size_t steps_bytes,
                              float *fitness, size_t fitness_bytes, uint32_t *generation, size_t generation_bytes);
int sots_batch_read_history(sots_batch *b, uint32_t chunk, sots_gen_record *out, uint32_t capacity, uint32_t *written,
                            uint64_t *taken);
/* ends at the first block boundary at which the rule holds for EVERY active chunk (the chunks advance together) */
int sots_batch_execute_until(sots_batch *b, uint32_t max_generations, const sots_stop_rule *rule, uint32_t *generations_run);

/* ---- chunk queue (new; extends parameterMatchAudio, Evolutionary_Strategy_OpenCL.hpp:572-610) ----
 * M chunks, any number, go through the S = min(max_chunks, M) slots of a tracked batch.  Every chunk runs under a
 * generation counter of its own until its own stop rule holds at one of its own check boundaries (multiples of
 * rule->check_interval, and max_generations) or until it has run max_generations; its result is then stored on the
 * device and its slot takes the next unstarted chunk, without the stream draining.  Chunk k's result is bit for bit what
 * a tracked sots_ctx of the same configuration reports after sots_set_target_spectrum(target k),
 * sots_init_population(ctx, first_chunk_index + k) and sots_execute_until(ctx, max_generations, rule, &run) - whichever
 * slot the chunk ran in and whenever it started. */
typedef struct sots_chunk_result {            /* 208 bytes */
    uint32_t generations_run;                 /* the chunk's own counter when it was retired */
    uint32_t best_ever_generation;
    float best_ever_fitness;
    float last_fitness;                       /* row 0 of the generation it stopped at */
    float best_ever_values[SOTS_MAX_DIMS];    /* entries >= D are 0 */
    float best_ever_steps[SOTS_MAX_DIMS];
    float last_values[SOTS_MAX_DIMS];         /* row 0 of the generation it stopped at */
} sots_chunk_result;
typedef struct sots_queue_stats {
    uint32_t struct_size;                     /* = sizeof(sots_queue_stats), set by the caller */
    uint32_t slots;                           /* min(max_chunks, num_chunks); with carried rows min(max_chunks, segments) */
    uint64_t global_generations;              /* generations the batch loop ran until the last chunk retired */
    uint64_t chunk_generations;               /* sum of generations_run */
} sots_queue_stats;
#define SOTS_QUEUE_NO_CHUNK 0xFFFFFFFFu
/* Store the targets of num_chunks >= 1 chunks on the device (as sots_batch_set_target_*: chunk k = bins [k N/2, (k+1) N/2)
 * / samples [k N, (k+1) N), the audio form through the same host transform, chunk by chunk).  The stored targets and
 * results are bounded by BYTES: num_chunks * N/2 * 4 <= 2^30 (262144 chunks at N = 2048), SOTS_ERR_INVALID above that.
 * num_bins == num_chunks * N/2 and num_samples >= num_chunks * N, else SOTS_ERR_SIZE.  Replaces an earlier queue. */
int sots_batch_queue_targets_spectra(sots_batch *b, const float *magnitudes, uint64_t num_bins, uint32_t num_chunks);
int sots_batch_queue_targets_audio(sots_batch *b, const float *audio, uint64_t num_samples, uint32_t num_chunks);
/* the audio form with chunk k = samples [k hop, k hop + N), 1 <= hop <= N (SOTS_ERR_INVALID otherwise);
 * num_samples >= (num_chunks - 1) hop + N, else SOTS_ERR_SIZE.  sots_batch_queue_targets_audio is its hop = N case. */
int sots_batch_queue_targets_audio_hop(sots_batch *b, const float *audio, uint64_t num_samples, uint32_t hop, uint32_t num_chunks);
/* Runs the stored queue; blocks until the last chunk is retired.  rule NULL: every chunk runs max_generations (>= 1).
 * max_generations need not be a multiple of rule->check_interval: a chunk's last block is the shorter one, as in
 * sots_execute_until.  keep_chunk (SOTS_QUEUE_NO_CHUNK: none; else < num_chunks): that chunk's whole current half, as it
 * was when the chunk was retired, is kept for sots_batch_queue_read_kept_population.  Needs SOTS_TRACK_BEST_EVER on the
 * batch and fails with SOTS_TRACK_HISTORY on (both SOTS_ERR_STATE: the slots keep no history rings), and needs targets
 * stored (SOTS_ERR_STATE).  Afterwards the batch has NO active targets: the ordinary sots_batch_* calls need
 * sots_batch_set_target_* again and then compute exactly what they compute on a fresh handle; the stored queue stays and
 * can be run again.  stats may be NULL. */
int sots_batch_queue_run(sots_batch *b, uint32_t first_chunk_index, uint32_t max_generations, const sots_stop_rule *rule,
                         uint32_t keep_chunk, sots_queue_stats *stats);
/* Carried rows (new): a setting {carry_rows R, segment_chunks L} of the batch that sots_batch_queue_run
 * alone reads.  The M queued chunks are cut into segments of L consecutive chunks, segment g = chunks [g L, min((g+1) L, M)).
 * Chunk k with k % L != 0 is a SUCCESSOR: it starts in the slot in which chunk k-1 has just been retired, in the same
 * launch, from this population:
 *   row 0          values and steps of chunk k-1's best-ever record, as its result holds them;
 *   rows 1..R-1    values and steps of rows 1..R-1 of chunk k-1's current (sorted) half as it was when retired;
 *   rows R..P-1    exactly what sots_init_population(first_chunk_index + k) draws for those rows;
 *   every fitness 0, the record cleared, the counter 0, the target chunk k's - all as without carrying.
 * A segment's first chunk (k % L == 0) starts exactly as without carrying.  A free slot draws the next unstarted SEGMENT;
 * S = min(max_chunks, ceil(M / L)) slots run, slot c starting with chunk c L, and sots_queue_stats.slots reports that S.
 * Chunk k's result depends on its predecessors in its segment only - not on the slot, on max_chunks or on when the
 * segment started.  It is bit for bit what a tracked sots_ctx with the same survivors setting reports from
 *     if (k % L) { (pv, ps) = sots_read_population; (bv, bs) = sots_read_best_ever; }          state left by chunk k-1
 *     sots_set_target_spectrum(target k); sots_init_population(first_chunk_index + k);
 *     if (k % L) { (v, s) = sots_read_population; v[0..R-1] = pv[0..R-1]; s[0..R-1] = ps[0..R-1]; v[0] = bv; s[0] = bs;
 *                  sots_write_population(v, s, no fitness); }
 *     sots_execute_until(max_generations, rule)
 * carry_rows 0 (the default) turns it off: segment_chunks is ignored and reported as 0, and a run enqueues the launches
 * and computes the bits it always did.  Otherwise 1 <= carry_rows <= numParents (recombination reads parent rows only: R
 * chooses how many of the first generation's parents are carried and how many are fresh) and segment_chunks >= 1 (1: no
 * chunk is a successor; larger than M: one segment); anything else is SOTS_ERR_INVALID and the old setting stays.
 * Without survivors the carried rows are only ingredients of the first recombination: use it with
 * sots_batch_set_survivors >= 1.  Targets, objective, weights, survivors and runs keep the setting;
 * sots_batch_execute_* ignores it.  With it the loop generations are bounded by segments of min(L, M) chunks:
 * ((ceil(M / L) - 1) / S + 2) L max_generations with a rule, ceil(ceil(M / L) / S) L max_generations without. */
int sots_batch_queue_set_carry(sots_batch *b, uint32_t carry_rows, uint32_t segment_chunks);
int sots_batch_queue_get_carry(const sots_batch *b, uint32_t *carry_rows, uint32_t *segment_chunks);
/* the results of the last run, chunk 0 first: *written = min(num_chunks, capacity).  SOTS_ERR_STATE before a run.  Blocking. */
int sots_batch_queue_results(sots_batch *b, sots_chunk_result *out, uint32_t capacity, uint32_t *written);
/* the kept chunk's population; pointers and byte counts as sots_read_population.  SOTS_ERR_STATE when the last run kept none. */
int sots_batch_queue_read_kept_population(sots_batch *b, float *values, size_t values_bytes, float *steps, size_t steps_bytes,
                                          float *fitness, size_t fitness_bytes);
/* The global generations an in-order refill of `slots` slots takes for these per-chunk counts: every slot starts at global
 * generation 0, chunks start in index order, and a freed slot starts the next chunk at the boundary at which it was freed
 * (which freed slot takes which chunk does not change the answer).  slots >= 1; num_chunks 0 gives 0.  Pure host code: no
 * device, no handle. */
int sots_queue_makespan(const uint32_t *generations_run, uint32_t num_chunks, uint32_t slots, uint64_t *global_generations);

/* ---- analysis on the device (new; the reference transforms every chunk on the host, Objective::calculateFFT,
 * Evolutionary_Strategy.hpp:524-542) ----
 * Frame f of a signal is its samples [f hop, f hop + N), 1 <= hop <= N.  The device analysis uploads the signal ONCE and
 * transforms every frame where it lies: the batch's fp32 window table, a real-input FFT in fp32, and for k < N/2
 * m_k = |X_k / N / windowFactor| - the magnitudes sots_batch_set_target_spectra and sots_batch_queue_targets_spectra take.
 * A frame's bits depend on its N samples only (not on hop, the frame count or its neighbours); a non-finite sample makes
 * the magnitudes of the frames that contain it non-finite, and of no other frame.
 *
 * THE DEVICE'S MAGNITUDES ARE NOT THE HOST'S BITS.  The host transform is fp64 rounded to fp32 at the end, the device's
 * is fp32 throughout: they agree to about 3e-6 of a frame's largest bin, and a population matched against one does not
 * repeat, bit for bit, a run against the other.  Hence a setting, off by default. */
enum sots_analysis { SOTS_ANALYSIS_HOST = 0, SOTS_ANALYSIS_DEVICE = 1 };
/* How the four audio target calls of the batch (sots_batch_set_target_audio[_hop], sots_batch_queue_targets_audio[_hop])
 * make their spectra.  HOST (the default): chunk by chunk on the host, every copy, launch and bit as before.  DEVICE: the
 * (num_chunks - 1) hop + N samples go up once, the device analysis writes the stored targets, and the call continues as its
 * spectra form does; then the samples are bounded as below (SOTS_ERR_INVALID beyond 2^28).  An unknown mode is
 * SOTS_ERR_INVALID and the old setting stays.  Targets already stored are not touched. */
int sots_batch_set_analysis(sots_batch *b, uint32_t mode);
int sots_batch_get_analysis(const sots_batch *b, uint32_t *mode);
/* The device analysis of num_frames frames, whatever the mode: magnitudes[num_frames][N/2] come back to the host,
 * num_bins == num_frames * N/2.  Blocking.  Population, targets, queue, run record and counters stay as they are; the
 * scratch is the batch's own and is freed with it.
 * SOTS_ERR_INVALID: a null pointer, hop outside 1..N, num_frames 0, (num_frames - 1) hop + N > 2^28 samples or
 * num_frames * N/2 * 4 > 2^30 bytes.  SOTS_ERR_SIZE: num_samples < (num_frames - 1) hop + N, or a wrong num_bins. */
int sots_batch_analyse_audio_hop(sots_batch *b, const float *audio, uint64_t num_samples, uint32_t hop, uint32_t num_frames,
                                 float *magnitudes, uint64_t num_bins);
/* Frame k of `audio` scored against STORED QUEUE TARGET k under the batch's objective, floor and weights:
 * fitness[k] = sum_j (u_j e_j)^2 with e_j the objective's signed error of bin j, summed in a fixed order (the same inputs
 * give the same bits run to run; they need not be the bits a spectral kernel gives a synthesised row).  A signal scored
 * against device-made targets of the same samples gives exactly 0.  Needs a stored queue (SOTS_ERR_STATE) of num_chunks
 * chunks (SOTS_ERR_SIZE); the other limits are those of sots_batch_analyse_audio_hop.  Blocking; changes nothing. */
int sots_batch_queue_score_audio_hop(sots_batch *b, const float *audio, uint64_t num_samples, uint32_t hop, float *fitness,
                                     uint32_t num_chunks);

/* ---- introspection ---- */
typedef struct sots_info {
    uint32_t population_length, num_dimensions, audio_length, spectrum_row_floats;
    uint32_t rotation_index, generation, compute_units, reserved;
    char device_name[128];
    char arch[32];
} sots_info;
int sots_get_info(const sots_ctx *ctx, sots_info *info);

#ifdef __cplusplus
}
#endif
#endif /* SOTS_HIP_H */
