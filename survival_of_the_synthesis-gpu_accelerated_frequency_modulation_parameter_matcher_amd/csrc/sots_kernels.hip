// sots_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels for the per-generation
// evolutionary FM sound-matching loop.  Compiled with -ffp-contract=off: every fp32
// expression rounds exactly as written, which is what makes synthesis, recombination and
// the value half of mutation bit-identical to the CPU restatement.
//
// Layout choices (DESIGN.md has the reasoning):
//   * variation kernels        : one lane per gene, coalesced [P][D] rows
//   * synthesisePopulation     : one lane per individual (the phase recurrence is serial in
//                                fp32), 128 KiB wavetable staged in LDS, 16-byte row stores
//   * FFT / fitness            : one individual per wavefront, Stockham radix-8/4 passes
//                                (three/two radix-2 layers kept in registers), padded LDS
//                                exchange, xor-shuffle reduction of the squared error
//   * sortPopulation           : bitonic network on (fitness, index) 64-bit keys, LDS tiles
//
// The one translation unit of the kernels, and host code only: launchers, launch rules and size functions.  Every kernel
// lives in a family header under csrc/kernels/, included here where its code stood, so the order of the
// definitions - and of the kernels in the object - is what it was.  A family file states its contraction mode in its first
// lines and ends with contract(off), this unit's default; no contraction pragma stands in this file.  stamps.h is included
// for sots_debug_stamps / sots_debug_clear_stamps at the end, which read g_stamps.
//
// Reference citations are file:line in the reference tree.
#include "sots_kernels.h"
#include "kernels/common.h"
#include "kernels/stamps.h"
#include <type_traits>

#include <cstdlib>

#include "kernels/variation.h"
#include "kernels/synth_common.h"
#include "kernels/synth_lanes.h"
#include "kernels/synth_ol.h"
#include "kernels/synth_tp.h"
#include "kernels/window.h"
#include "kernels/fft.h"
#include "kernels/objective.h"
#include "kernels/sel_keys.h"
#include "kernels/spectral_wave.h"
#include "kernels/sort.h"
#include "kernels/select_tiles.h"
#include "kernels/select_splitters.h"
#include "kernels/spectral_x.h"
#include "kernels/spectral_big.h"
#include "kernels/exchange.h"

namespace sots {

uint32_t next_pow2(uint32_t v)
{
    uint32_t r = 1;
    while (r < v) r <<= 1;
    return r;
}

namespace {

inline uint32_t grid_for(uint64_t work, uint32_t threads, uint32_t cap = 2048)
{
    uint64_t g = (work + threads - 1) / threads;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (uint32_t)g;
}

} // namespace

// ------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------
hipError_t launch_init_population(hipStream_t st, float *values, float *steps, float *fitness,
                                  const PopDims &pd, uint32_t chunk)
{
    k_init_population<<<grid_for((uint64_t)pd.p * pd.d, 256), 256, 0, st>>>(values, steps, fitness, pd, chunk);
    return hipGetLastError();
}

hipError_t launch_recombine(hipStream_t st, const float *vin, const float *sin, float *vout, float *sout,
                            const PopDims &pd)
{
    k_recombine<<<grid_for((uint64_t)pd.p * pd.d, 256), 256, 0, st>>>(vin, sin, vout, sout, pd);
    return hipGetLastError();
}

hipError_t launch_mutate(hipStream_t st, float *values, float *steps, const PopDims &pd,
                         const MutateConsts &mc, uint32_t generation)
{
    k_mutate<<<grid_for((uint64_t)pd.p * pd.d, 256), 256, 0, st>>>(values, steps, pd, mc, generation);
    return hipGetLastError();
}

hipError_t launch_recombine_mutate(hipStream_t st, const float *vin, const float *sin, float *vout,
                                   float *sout, const PopDims &pd, const MutateConsts &mc,
                                   uint32_t generation)
{
    k_recombine_mutate<<<grid_for((uint64_t)pd.p * pd.d, 256), 256, 0, st>>>(vin, sin, vout, sout, pd, mc,
                                                                               generation);
    return hipGetLastError();
}

// Where k_synth_tp runs: at most 16 individuals per CU for the 2-operator voice (populations up to 4096; 22-27 us of
// synthesis against 32-35 at N = 1024; beyond that k_synth's cut kernels win), 12 / 9 / 5 for 3 / 4 operators in series /
// three parallel chains (what fits beside the table)
#ifndef SOTS_TP_2OP_MAX
#define SOTS_TP_2OP_MAX 16
#endif
#ifndef SOTS_OL_MIN_SHARE
#define SOTS_OL_MIN_SHARE 48
#endif
// Where k_synth_ol runs (same-box A/Bs, profiles/r04_experiments.md): the 4-operator voice from 65 individuals per CU (65 ... 240
// in one tile: 128 per CU 146-157 against 189 us, 192 per CU 199 against 297; beyond that in equal tiles: 256 per CU 302-307 against 313-317 + the
// variation launch, 313 per CU 389 against 612), the 3-operator voice at 65 ... 240 (128 per CU 91 against 95, 192 per CU 106 against
// 128; at 256 and 512 per CU k_synth wins: 126 against 152, 254 against 310)
bool synth_operators_in_lanes(uint32_t kind, uint32_t p, uint32_t num_cus)
{
#ifdef SOTS_SYNTH_NO_OL
    return false;
#else
    const uint32_t cus = num_cus ? num_cus : 256u, share = (p + cus - 1) / cus;
    if (kind == SOTS_SYNTH_4OP_SERIES) return share > 64u;
    if (kind == SOTS_SYNTH_3OP_SERIES) return share > 64u && share <= (uint32_t)kOlTileRows;
    return false;
#endif
}
bool synth_time_parallel(uint32_t kind, uint32_t p, uint32_t num_cus)
{
#ifdef SOTS_SYNTH_NO_TP
    return false;
#else
    const uint32_t share = (p + (num_cus ? num_cus : 256u) - 1) / (num_cus ? num_cus : 256u);
    switch (kind) {
    case SOTS_SYNTH_2OP: return share <= (uint32_t)SOTS_TP_2OP_MAX;
    case SOTS_SYNTH_3OP_SERIES: return share <= (uint32_t)tp_max_individuals<SOTS_SYNTH_3OP_SERIES>();
    case SOTS_SYNTH_4OP_SERIES: return share <= (uint32_t)tp_max_individuals<SOTS_SYNTH_4OP_SERIES>();
    case SOTS_SYNTH_TRIPLE_PAR: return share <= (uint32_t)tp_max_individuals<SOTS_SYNTH_TRIPLE_PAR>();
    default: return false;
    }
#endif
}

} // namespace sots

#include "kernels/synth_dev.h"

namespace sots {

hipError_t launch_synth_device_arith(hipStream_t st, uint32_t kind, const float *values, const float *wavetable, float *audio,
                                     const SynthParams &sp, uint32_t p, uint32_t log2n, uint32_t pitch)
{
    const uint32_t n = 1u << log2n, grid = (p + 255u) / 256u;
    switch (kind) {
    case SOTS_SYNTH_2OP: k_synth_dev<SOTS_SYNTH_2OP><<<grid, 256, 0, st>>>(values, wavetable, audio, sp, p, n, pitch); break;
    case SOTS_SYNTH_3OP_SERIES: k_synth_dev<SOTS_SYNTH_3OP_SERIES><<<grid, 256, 0, st>>>(values, wavetable, audio, sp, p, n, pitch); break;
    case SOTS_SYNTH_TRIPLE_PAR: k_synth_dev<SOTS_SYNTH_TRIPLE_PAR><<<grid, 256, 0, st>>>(values, wavetable, audio, sp, p, n, pitch); break;
    default: return hipErrorInvalidValue; // (the 4-op voice is build-defined: the reference has no kernel to agree with)
    }
    return hipGetLastError();
}

hipError_t launch_synth(hipStream_t st, uint32_t kind, const float *values, const float *wavetable,
                        float *audio, const SynthParams &sp, uint32_t p, uint32_t log2n, uint32_t pitch,
                        uint32_t num_cus, const Variation *variation, bool allow_cut, const sots_voice_graph *graph,
                        uint32_t waveforms, const float *feedback, uint32_t feedback_genes)
{
    // the operator-graph voice has one kernel form, in a file of its own; it makes no individuals
    if (kind == SOTS_SYNTH_GRAPH) {
        if (!graph || variation) return hipErrorInvalidValue;
        return launch_synth_graph(st, *graph, values, wavetable, audio, sp, p, log2n, pitch, num_cus, waveforms, feedback, feedback_genes);
    }
    Variation var = {};
    if (variation) var = *variation;
    const uint32_t n = 1u << log2n;
    const uint32_t cus = num_cus ? num_cus : 256;
    // The 128 KiB table allows one workgroup per CU, so the workgroup is sized to the CU's share
    // of the population, up to one wavefront per SIMD; larger populations loop.  Up to two
    // wavefronts' worth per CU, a series voice is cut into two wavefronts per 64 individuals.
    const uint32_t share = (p + cus - 1) / cus;
    // a few individuals per CU: the time axis in the lanes (k_synth_tp), two wavefronts per operator
    if (allow_cut && synth_time_parallel(kind, p, num_cus)) {
        switch (kind) {
        case SOTS_SYNTH_2OP: k_synth_tp<SOTS_SYNTH_2OP><<<(p + share - 1) / share, tp_waves<SOTS_SYNTH_2OP>() * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, share, var); break;
        case SOTS_SYNTH_3OP_SERIES: k_synth_tp<SOTS_SYNTH_3OP_SERIES><<<(p + share - 1) / share, tp_waves<SOTS_SYNTH_3OP_SERIES>() * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, share, var); break;
        case SOTS_SYNTH_TRIPLE_PAR: k_synth_tp<SOTS_SYNTH_TRIPLE_PAR><<<(p + share - 1) / share, tp_waves<SOTS_SYNTH_TRIPLE_PAR>() * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, share, var); break;
        default: k_synth_tp<SOTS_SYNTH_4OP_SERIES><<<(p + share - 1) / share, tp_waves<SOTS_SYNTH_4OP_SERIES>() * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, share, var); break;
        }
        return hipGetLastError();
    }
    // The 3- and 4-operator voices from 65 individuals per CU (BASELINE configs[3]'s shard: 128): the operators in the lanes
    // (k_synth_ol; where exactly: synth_operators_in_lanes above) - every wavefront carries 16 individuals, up to fifteen wavefronts per
    // CU without hand-overs or barriers.  The 2-operator voice stays on k_synth (224 per CU: 49.3 against 51.1 us, and 256 per CU - BASELINE
    // configs[2] - leaves no LDS for the spare table entry and the progress counters); `SOTS_OL_ALL` is an experiment switch.
#ifndef SOTS_SYNTH_NO_OL
#ifdef SOTS_OL_ALL
    const bool use_ol = allow_cut && kind != SOTS_SYNTH_TRIPLE_PAR && share >= (uint32_t)SOTS_OL_MIN_SHARE;
#else
    const bool use_ol = allow_cut && synth_operators_in_lanes(kind, p, num_cus);
#endif
    if (use_ol) {
        auto launch_ol = [&](auto kind_tag) {
            constexpr int K = decltype(kind_tag)::value, OPS = VoiceShape<K>::OPS, IPW = OlShape<OPS>::IPW;
            constexpr uint32_t max_rows = ol_max_waves<OPS>() * IPW;
            // a CU's share in equal tiles of at most max_rows rows (256 per CU: two tiles of 128, not 240 + 16)
            const uint32_t tiles_per_cu = (share + max_rows - 1) / max_rows;
            uint32_t rows = ((share + tiles_per_cu - 1) / tiles_per_cu + IPW - 1) / IPW * IPW;
            rows = rows > max_rows ? max_rows : rows;
            uint32_t grid = (p + rows - 1) / rows;
            grid = grid > cus ? cus : grid; // larger populations: a workgroup takes several tiles
            k_synth_ol<K><<<grid, rows / IPW * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        };
        switch (kind) {
        case SOTS_SYNTH_2OP: launch_ol(ic<SOTS_SYNTH_2OP>{}); break;
        case SOTS_SYNTH_3OP_SERIES: launch_ol(ic<SOTS_SYNTH_3OP_SERIES>{}); break;
        default: launch_ol(ic<SOTS_SYNTH_4OP_SERIES>{}); break;
        }
        return hipGetLastError();
    }
#endif
    uint32_t waves = (share + kWave - 1) / kWave;
    waves = waves < 1 ? 1 : waves > (uint32_t)kSynthWaves ? (uint32_t)kSynthWaves : waves;
    const bool cut = allow_cut && waves <= 2 && kind != SOTS_SYNTH_TRIPLE_PAR;
    const uint32_t threads = (cut ? 2 : 1) * waves * kWave, grid = grid_for(p, waves * kWave, cus);
    // variation folded in, 2-operator voice, full workgroups with one tile each: sixteen wavefronts make the individuals
    if (var.vin && kind == SOTS_SYNTH_2OP && !cut && (uint64_t)grid * waves * kWave * 2 >= p) { // one or two tiles per workgroup
        k_synth<SOTS_SYNTH_2OP, 0, true><<<grid, 4 * waves * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        return hipGetLastError();
    }
    // ... and the cut kernels of a small population likewise: four threads per individual make the genes (one, two or three
    // each), then a wavefront per stage and 64 individuals stays (one tile per workgroup there)
    if (var.vin && cut && (uint64_t)grid * waves * kWave >= p) {
        const uint32_t ht = 4 * waves * kWave;
        switch (kind) {
        case SOTS_SYNTH_2OP: k_synth<SOTS_SYNTH_2OP, 1, true><<<grid, ht, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var); return hipGetLastError();
        // up to 64 individuals per CU every operator of a 3- or 4-operator chain gets a wavefront of its own (three or four
        // SIMDs busy; a stage is one operator long: 3-op N = 2048 P = 1024 105 -> 81 us per generation, 4-op N = 4096 204 -> 170)
        case SOTS_SYNTH_3OP_SERIES:
            if (waves == 1) k_synth<SOTS_SYNTH_3OP_SERIES, 1, true, 2><<<grid, ht, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
            else k_synth<SOTS_SYNTH_3OP_SERIES, 2, true><<<grid, ht, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
            return hipGetLastError();
        case SOTS_SYNTH_4OP_SERIES:
            if (waves == 1) k_synth<SOTS_SYNTH_4OP_SERIES, 1, true, 2, 3><<<grid, ht, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
            else k_synth<SOTS_SYNTH_4OP_SERIES, 1, true, 2, 3><<<grid, ht, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var); // (all eight wavefronts stay)
            return hipGetLastError();
        default: break;
        }
    }
#define SOTS_SYNTH_CASE(K, S)                                                                            \
    case K:                                                                                              \
        if (cut) k_synth<K, S><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var); \
        else k_synth<K, 0><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);     \
        break;
    switch (kind) {
        SOTS_SYNTH_CASE(SOTS_SYNTH_2OP, 1)
    case SOTS_SYNTH_3OP_SERIES:
        // one group of 64 per CU: a wavefront per operator (three SIMDs); two groups: the chain cut once (four wavefronts)
        if (cut && waves == 1) k_synth<SOTS_SYNTH_3OP_SERIES, 1, false, 2><<<grid, 3 * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        else if (cut) k_synth<SOTS_SYNTH_3OP_SERIES, 2><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        else k_synth<SOTS_SYNTH_3OP_SERIES, 0><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        break;
    case SOTS_SYNTH_4OP_SERIES:
        // up to 128 individuals per CU a wavefront per operator: four wavefronts for one group of 64 (round 2: three stages
        // {0, 1} | {2} | {3} with 16-sample blocks: 165 against 131 us at P = 1024, N = 4096), eight for two (BASELINE configs[3]'s
        // shard; `-DSOTS_SYNTH_NO_CUT3`: the single cut of round 2 there)
#ifndef SOTS_SYNTH_NO_CUT3
        if (cut) k_synth<SOTS_SYNTH_4OP_SERIES, 1, false, 2, 3><<<grid, 4 * waves * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
#else
        if (cut && waves == 1) k_synth<SOTS_SYNTH_4OP_SERIES, 1, false, 2, 3><<<grid, 4 * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        else if (cut) k_synth<SOTS_SYNTH_4OP_SERIES, 2><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
#endif
        else k_synth<SOTS_SYNTH_4OP_SERIES, 0><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        break;
    case SOTS_SYNTH_TRIPLE_PAR:
        // up to 64 individuals per CU a wavefront per chain (three SIMDs): 134 -> ... us at P = 1024 (profiles/r03_experiments.md)
        if (allow_cut && waves == 1) k_synth<SOTS_SYNTH_TRIPLE_PAR, -1><<<grid, 3 * kWave, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        else k_synth<SOTS_SYNTH_TRIPLE_PAR, 0><<<grid, threads, 0, st>>>(values, wavetable, audio, sp, p, n, pitch, var);
        break;
    default: return hipErrorInvalidValue;
    }
#undef SOTS_SYNTH_CASE
    return hipGetLastError();
}

hipError_t launch_window(hipStream_t st, float *audio, const float *window, uint32_t p, uint32_t log2n,
                         uint32_t pitch)
{
    const size_t total4 = ((size_t)p << log2n) / 4;
    k_window<<<grid_for(total4, 256, 8192), 256, 0, st>>>(audio, window, total4, log2n - 2, pitch / 4);
    return hipGetLastError();
}

// Grid of a grid-stride kernel whose items all cost the same: exactly as many workgroups as
// are resident at once (occupancy query, cached per kernel and per context: OccCache).  A larger grid runs in rounds
// and the last, partly filled round costs as much as a full one (measured: 4096 one-wave
// workgroups on 3072 slots took 1.5x the time of 3072).
template <typename K>
static uint32_t resident_grid(K kernel, int threads, uint32_t items, uint32_t num_cus, int *cache)
{
    if (*cache == 0) {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess || per_cu < 1) per_cu = 1;
        *cache = per_cu;
    }
    const uint64_t cap = (uint64_t)(num_cus ? num_cus : 256) * (uint64_t)*cache;
    // (a grid balanced to equal row counts - 2979 workgroups of 22 rows instead of 3072 of 21 or 22 at P = 65536 - measures
    // the same: profiles/r03_experiments.md)
    return (uint32_t)(items < cap ? items : cap);
}

// The occupancy query of resident_grid and the launch: a call site names its instantiation once, as a function pointer
template <typename... KA, typename... A>
static hipError_t launch_resident(void (*kernel)(KA...), int threads, uint32_t items, uint32_t num_cus, int *cache, hipStream_t st, A... args)
{
    kernel<<<resident_grid(kernel, threads, items, num_cus, cache), threads, 0, st>>>(args...);
    return hipGetLastError();
}
constexpr uint32_t groups_of(uint32_t rows, uint32_t waves) { return (rows + waves - 1) / waves; } // workgroups of `waves` rows

// Which N has which kernel, each list written once (the lists decide what is instantiated): N <= 1024 runs on the
// wavefront-per-row kernels with LDS exchanges (k_fft, k_fitness), longer rows - and N = 256 (round 4): two complex points
// per lane, where k_fft's radix-4 / radix-8 passes need four or eight - on the wavefront-per-row kernels with the
// sub-transforms across lanes (k_fft_x, k_fitness_x; N = 1024 is instantiated for -DSOTS_X_MIN=10), N >= 16384 on the
// workgroup-per-row kernels (k_fft_big, k_fitness_big)
template <int... Ls> struct Log2nList {};
using WaveSizes = Log2nList<9, 10>;
using XSizes = Log2nList<8, 10, 11, 12, 13>;
using BigSizes = Log2nList<14, 15>;
// f(ic<L>{}) for the L of the list that equals log2n; `none` where the list has no such L.  (A left fold: f is instantiated
// in list order, and the order in which the launchers below first name the kernels is their order in the code object)
template <int... Ls, typename R, typename F>
static R for_log2n(Log2nList<Ls...>, uint32_t log2n, R none, F f)
{
    (void)(... || (log2n == (uint32_t)Ls && ((void)(none = f(ic<Ls>{})), true)));
    return none;
}
template <typename List> static bool has_log2n(List list, uint32_t log2n) { return for_log2n(list, log2n, false, [](auto) { return true; }); }

#ifndef SOTS_X_MIN
#define SOTS_X_MIN 11
#endif
static bool x_from(uint32_t log2n) { return has_log2n(XSizes{}, log2n) && (log2n == 8 || log2n >= SOTS_X_MIN); }
static bool big_from(uint32_t log2n) { return has_log2n(BigSizes{}, log2n); }

// N = 1024 from one row per resident wavefront (P >= 12 x CUs): one workgroup of twelve wavefronts per CU, rows dealt as
// the wavefronts ask (k_fft); 15.7 -> 14.7 us at P = 8192 already, level at 4096
static bool fft_wide(uint32_t p, uint32_t log2n, uint32_t num_cus)
{
#ifdef SOTS_FFT_NO_WIDE
    return false; // (experiments: the one-wavefront workgroups at every size)
#else
#ifndef SOTS_FFT_WIDE_ROWS
#define SOTS_FFT_WIDE_ROWS 1u
#endif
    return log2n == 10 && p >= SOTS_FFT_WIDE_ROWS * fft_wide_waves<10>() * (num_cus ? num_cus : 256u);
#endif
}

// The kernel choice of every spectral launcher, plain or segmented, staged or fused.  x_small: a small population, a
// wavefront per SIMD (k_fft_x with four wavefronts; the fused windowed form only, the others take it as x).  The threshold
// (fewer 16-row workgroups than CUs) was measured at N = 4096 and 2048, where x_waves is 16; N = 8192 (x_waves 8) follows
// it unmeasured
enum class Spectral { none, wave, wide, x, x_small, big };
static Spectral spectral_choice(uint32_t p, uint32_t log2n, uint32_t num_cus)
{
    if (big_from(log2n)) return Spectral::big;
    if (x_from(log2n)) return groups_of(p, x_waves<12>()) < (num_cus ? num_cus : 256u) ? Spectral::x_small : Spectral::x;
    if (fft_wide(p, log2n, num_cus)) return Spectral::wide;
    return has_log2n(WaveSizes{}, log2n) ? Spectral::wave : Spectral::none;
}

// The lookup of every launch that files keys (kernels/sel_keys.h), the spectral kernel's and the staged k_bucket_fitness's
// alike, so that a staged and a fused run of one population file by the same code: two levels up to 65 536 rows, where they
// won every round (1.4-1.5 us of 113-115 per generation, profiles/r30_experiments.md), all bounds against every key above,
// where the two levels lost 4.4 us of 212 at 131 072 rows (profiles/r19_experiments.md).  The buckets are the same either way.
#ifndef SOTS_BKT_TWO_LEVEL_MAX_P
#define SOTS_BKT_TWO_LEVEL_MAX_P 65536u // (0u: the build variant that files flat at every size)
#endif
static bool bkt_two_level(uint32_t p) { return p <= SOTS_BKT_TWO_LEVEL_MAX_P; }

// a workgroup per row: as many workgroups as rows, at most four per CU (they loop)
static uint32_t big_grid(uint32_t p, uint32_t num_cus)
{
    const uint32_t cap = 4u * (num_cus ? num_cus : 256u);
    return p < cap ? p : cap;
}
template <int L, int MODE, bool WIN, bool SEG = false, int OBJ = kObjMagnitude, bool WGT = false, typename... FL>
static hipError_t launch_fft_big(hipStream_t st, uint32_t p, uint32_t num_cus, const float *audio, float *spectrum, const float *target,
                                 float *fitness, const float2 *tw, const float *window, float inv_n, float inv_wf, uint32_t pitch, FL... fl)
{
    const auto kernel = k_fft_big<L, MODE, WIN, SEG, OBJ, WGT, FL...>;
    const size_t lds = ((size_t)(1u << L) / 2u) * sizeof(float2) + 64u;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    kernel<<<big_grid(p, num_cus), kBigThreads, lds, st>>>(audio, spectrum, target, fitness, tw, window, p, inv_n, inv_wf, pitch, fl...);
    return hipGetLastError();
}

hipError_t launch_fft(hipStream_t st, const float *audio, float *spectrum, const float2 *twiddle,
                      uint32_t p, uint32_t log2n, uint32_t pitch, uint32_t num_cus, OccCache *oc)
{
    constexpr int W = fft_wide_waves<10>();
    switch (spectral_choice(p, log2n, num_cus)) {
    case Spectral::big:
        return for_log2n(BigSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
            return launch_fft_big<decltype(l)::value, 0, false>(st, p, num_cus, audio, spectrum, nullptr, nullptr, twiddle, nullptr, 0.f, 0.f, pitch);
        });
    case Spectral::wide:
        return launch_resident(k_fft<10, 0, false, W>, W * kWave, groups_of(p, W), num_cus, &oc->wide[0], st, audio, spectrum, nullptr, nullptr, twiddle, nullptr, p, 0.f, 0.f, pitch);
    case Spectral::x_small: // (no four-wavefront form)
    case Spectral::x:
        return for_log2n(XSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
            constexpr int L = decltype(l)::value, WG = x_waves<L, 0>();
            return launch_resident(k_fft_x<L, 0, false>, WG * kWave, groups_of(p, WG), num_cus, &oc->x_fft[L], st, audio, spectrum, nullptr, nullptr, twiddle, nullptr, p, 0.f, 0.f, pitch, nullptr);
        });
    case Spectral::wave:
        return for_log2n(WaveSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
            constexpr int L = decltype(l)::value;
            return launch_resident(k_fft<L, 0, false>, kWave, p, num_cus, &oc->fft[L], st, audio, spectrum, nullptr, nullptr, twiddle, nullptr, p, 0.f, 0.f, pitch);
        });
    default: return hipErrorInvalidValue;
    }
}

// The objective and the weights of a launch as template arguments: f(ic<OBJ>{}, bool_constant<WGT>{}, fl...), where fl holds
// the log objective's floor and then the weighted kernels' table u (the kernels' last arguments); the unweighted magnitude
// instantiations are launched exactly as before there was a choice
template <typename F>
static hipError_t with_objective(const Objective &obj, const float *u, F f)
{
    if (obj.kind == SOTS_OBJECTIVE_LOG_MAGNITUDE) {
        if (u) return f(ic<kObjLogMagnitude>{}, std::true_type{}, obj.floor, u);
        return f(ic<kObjLogMagnitude>{}, std::false_type{}, obj.floor);
    }
    if (obj.kind != SOTS_OBJECTIVE_MAGNITUDE) return hipErrorInvalidValue;
    if (u) return f(ic<kObjMagnitude>{}, std::true_type{}, u);
    return f(ic<kObjMagnitude>{}, std::false_type{});
}

hipError_t launch_fitness(hipStream_t st, const float *spectrum, const float *target, float *fitness,
                          uint32_t p, uint32_t log2n, float inv_n, float inv_wf, uint32_t num_cus, OccCache *oc, const Objective &obj)
{
    // (the staged kernels index the plain weight table by bin)
    return with_objective(obj, obj.weights, [&](auto o, auto w, auto... fl) {
        constexpr int OBJ = decltype(o)::value;
        constexpr bool WGT = decltype(w)::value;
        switch (spectral_choice(p, log2n, num_cus)) {
        case Spectral::big:
            return for_log2n(BigSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
                k_fitness_big<decltype(l)::value, OBJ, WGT, decltype(fl)...><<<big_grid(p, num_cus), kBigThreads, 0, st>>>(spectrum, target, fitness, p, inv_n, inv_wf, fl...);
                return hipGetLastError();
            });
        case Spectral::x_small: // (no four-wavefront form)
        case Spectral::x:
            return for_log2n(XSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
                constexpr int L = decltype(l)::value, WG = x_waves<L>();
                return launch_resident(k_fitness_x<L, OBJ, WGT, decltype(fl)...>, WG * kWave, groups_of(p, WG), num_cus, &oc->x_fitness[L], st, spectrum, target, fitness, p, inv_n, inv_wf, fl...);
            });
        case Spectral::wide: // (a wavefront per workgroup at every population)
        case Spectral::wave:
            return for_log2n(WaveSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
                constexpr int L = decltype(l)::value;
                return launch_resident(k_fitness<L, OBJ, WGT, decltype(fl)...>, kWave, p, num_cus, &oc->fitness[L], st, spectrum, target, fitness, p, inv_n, inv_wf, fl...);
            });
        default: return hipErrorInvalidValue;
        }
    });
}

hipError_t launch_objective_map(hipStream_t st, float *dst, const float *src, size_t n, float floor)
{
    if (n == 0) return hipSuccess;
    k_objective_map<<<grid_for(n, 256, 8192), 256, 0, st>>>(dst, src, n, floor);
    return hipGetLastError();
}

// the table image the fused long-row kernel copies in (bytes: x_table_bytes; rebuilt whenever the target changes)
size_t x_table_bytes(uint32_t log2n)
{
    return for_log2n(XSizes{}, log2n, (size_t)0, [](auto l) {
        constexpr int L = decltype(l)::value;
        return x_applies<L>() ? x_table_floats<L>() * sizeof(float) : (size_t)0; // (N = 256 makes its tables in the workgroup)
    });
}
hipError_t launch_x_tables(hipStream_t st, float *image, const float2 *twiddle, const float *window, const float *target, uint32_t log2n)
{
    if (!x_from(log2n)) return hipSuccess;
    hipError_t e = hipMemsetAsync(image, 0, x_table_bytes(log2n), st); // (the padding between the lanes' rows)
    if (e != hipSuccess) return e;
    return for_log2n(XSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
        k_x_tables<decltype(l)::value><<<8, 256, 0, st>>>(image, twiddle, window, target);
        return hipGetLastError();
    });
}

// The fused launch, plain (SEG = false: `target` is the one target, or the table image of k_fft_x) or segmented (every row
// against its chunk's target in the image `target`): one routine, so the same kernel choice for the same row count, and the
// same OccCache slots.  The forms without a window exist for the plain unweighted magnitude objective only (RAW; the library
// itself always passes its window; the log N = 4096 form without one would not fit its 128 registers): elsewhere a missing
// window is an error, not another kernel.  `lists`: the bucketing instantiation (plain only), or nothing - a caller that
// counts on the lists must not get a launch without them
template <bool SEG, int OBJ, bool WGT, typename... FL>
static hipError_t launch_fused(hipStream_t st, const float *audio, const float *window, const float *target, float *fitness,
                               const float2 *twiddle, uint32_t p, uint32_t log2n, uint32_t pitch, float inv_n, float inv_wf,
                               uint32_t num_cus, OccCache *oc, const SelLists *lists, FL... fl)
{
    constexpr bool RAW = !SEG && OBJ == kObjMagnitude && !WGT;
    constexpr int W = fft_wide_waves<10>();
    if (!RAW && !window) return hipErrorInvalidValue;
    if (lists) {
        if constexpr (SEG) return hipErrorInvalidValue;
        else {
            if (!window || !select_lists_apply(p, log2n, num_cus) || lists->buckets != select_splitter_count(num_cus) || !lists->slot || !lists->cnt || !lists->lists)
                return hipErrorInvalidValue;
            const auto file = [&](auto l) { // (l: the lists, typed by the lookup)
                return launch_resident(k_fft<10, 1, true, W, false, true, OBJ, WGT, decltype(l), FL...>, W * kWave, groups_of(p, W), num_cus, &oc->wide[3], st,
                                       audio, nullptr, target, fitness, twiddle, window, p, inv_n, inv_wf, pitch, l, fl...);
            };
            return bkt_two_level(p) ? file(SelListsTwoLevel{*lists}) : file(*lists);
        }
    }
    // f(bool_constant<WIN>{}): with the window, or without one where that form exists
    const auto with_window = [&](auto f) {
        if (window) return f(std::true_type{});
        if constexpr (RAW) return f(std::false_type{});
        return hipErrorInvalidValue;
    };
    const Spectral choice = spectral_choice(p, log2n, num_cus);
    switch (choice) {
    case Spectral::big: // (size outside, window inside: the order of these kernels in the code object)
        return for_log2n(BigSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
            return with_window([&](auto win) {
                return launch_fft_big<decltype(l)::value, 1, decltype(win)::value, SEG, OBJ, WGT, FL...>(st, p, num_cus, audio, nullptr, target, fitness, twiddle, window, inv_n, inv_wf, pitch, fl...);
            });
        });
    case Spectral::x_small:
    case Spectral::x:
        return with_window([&](auto win) {
            constexpr bool WIN = decltype(win)::value;
            if constexpr (WIN) { // (no four-wavefront form without a window)
                if (choice == Spectral::x_small)
                    return for_log2n(XSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
                        constexpr int L = decltype(l)::value;
                        return launch_resident(k_fft_x<L, 1, true, 4, SEG, OBJ, WGT, FL...>, 4 * kWave, groups_of(p, 4), num_cus, &oc->x_small[L], st,
                                               audio, nullptr, target, fitness, twiddle, window, p, inv_n, inv_wf, pitch, oc->x_image, fl...);
                    });
            }
            return for_log2n(XSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
                constexpr int L = decltype(l)::value, WG = x_waves<L>();
                return launch_resident(k_fft_x<L, 1, WIN, WG, SEG, OBJ, WGT, FL...>, WG * kWave, groups_of(p, WG), num_cus, WIN ? &oc->x_fused_win[L] : &oc->x_fused_raw[L], st,
                                       audio, nullptr, target, fitness, twiddle, window, p, inv_n, inv_wf, pitch, WIN ? oc->x_image : nullptr, fl...);
            });
        });
    case Spectral::wide:
        return with_window([&](auto win) {
            constexpr bool WIN = decltype(win)::value;
            return launch_resident(k_fft<10, 1, WIN, W, SEG, false, OBJ, WGT, FL...>, W * kWave, groups_of(p, W), num_cus, &oc->wide[WIN ? 1 : 2], st,
                                   audio, nullptr, target, fitness, twiddle, window, p, inv_n, inv_wf, pitch, fl...);
        });
    case Spectral::wave:
        return with_window([&](auto win) {
            constexpr bool WIN = decltype(win)::value;
            return for_log2n(WaveSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
                constexpr int L = decltype(l)::value;
                return launch_resident(k_fft<L, 1, WIN, 1, SEG, false, OBJ, WGT, FL...>, kWave, p, num_cus, WIN ? &oc->fused_win[L] : &oc->fused_raw[L], st,
                                       audio, nullptr, target, fitness, twiddle, window, p, inv_n, inv_wf, pitch, fl...);
            });
        });
    default: return hipErrorInvalidValue;
    }
}

// obj.weights_image holds u in the layout of the kernel's target table (one table for all chunks of a segmented launch)
template <bool SEG>
static hipError_t launch_fused_objective(hipStream_t st, const float *audio, const float *window, const float *target, float *fitness,
                                         const float2 *twiddle, uint32_t p, uint32_t log2n, uint32_t pitch, float inv_n, float inv_wf,
                                         uint32_t num_cus, OccCache *oc, const SelLists *lists, const Objective &obj)
{
    if (obj.weights && !obj.weights_image) return hipErrorInvalidValue;
    return with_objective(obj, obj.weights ? weight_table(obj.weights_image) : nullptr, [&](auto o, auto w, auto... fl) {
        return launch_fused<SEG, decltype(o)::value, decltype(w)::value>(st, audio, window, target, fitness, twiddle, p, log2n, pitch, inv_n, inv_wf, num_cus, oc, lists, fl...);
    });
}

hipError_t launch_fft_fitness(hipStream_t st, const float *audio, const float *window, const float *target,
                              float *fitness, const float2 *twiddle, uint32_t p, uint32_t log2n, uint32_t pitch,
                              float inv_n, float inv_wf, uint32_t num_cus, OccCache *oc, const SelLists *lists, const Objective &obj)
{
    return launch_fused_objective<false>(st, audio, window, target, fitness, twiddle, p, log2n, pitch, inv_n, inv_wf, num_cus, oc, lists, obj);
}

constexpr uint32_t kSortMaxTiles = 256;
constexpr uint32_t kSortTwoLevelFrom = 131072; // padded population from which runs of 8 tiles are merged first

// Plans: one LDS tile (n_pad <= 4096); tiles of 1024 + one rank level (up to 65536: 64 tiles);
// tiles of 1024 merged into runs of 8192 + a rank level over the runs (two levels: the rank work is
// quadratic in the number of sorted pieces, 128 tiles -> 16 runs at 131072); beyond 128 runs
// (n_pad > 1M) global bitonic steps over tiles of 4096.
constexpr uint32_t kSortMaxRuns = 128;         // 1 Mi keys; the counts of the run level take runs * n_pad * 2 bytes
static bool sort_two_level(uint32_t n_pad) { return n_pad >= kSortTwoLevelFrom && n_pad / kRankLdsKeys <= kSortMaxRuns; }

static void sort_plan(uint32_t n_pad, uint32_t &tile, uint32_t &tiles)
{
    if (n_pad <= kSortSmall) tile = n_pad; // (k_sort_small: no tiles at all)
    else if (n_pad <= 65536u || sort_two_level(n_pad)) tile = 1024u;
    else tile = kSortTile;
    tiles = n_pad / tile;
}

// tiles staged per rank workgroup: as many as fit the LDS buffer and a 16-bit count
static uint32_t rank_group(uint32_t tile, uint32_t tiles)
{
    uint32_t group = kRankLdsKeys / tile;
    if (group > kRankGroup) group = kRankGroup;
    if (group < 1) group = 1;
    while (group > tiles) group >>= 1;
    return group;
}

// scratch layout: [partial counts (u16)] then, for two levels, [merged runs (u64, n_pad keys)]
static size_t sort_partial_bytes(uint32_t n_pad)
{
    uint32_t tile, tiles;
    sort_plan(n_pad, tile, tiles);
    if (sort_two_level(n_pad)) return (size_t)(n_pad / kRankLdsKeys) * n_pad * sizeof(uint16_t);
    if (tiles <= 1 || tiles > kSortMaxTiles) return 16;
    const uint32_t group = rank_group(tile, tiles);
    return (size_t)(tiles / group) * n_pad * sizeof(uint16_t);
}

size_t sort_scratch_bytes(uint32_t p)
{
    const uint32_t n_pad = next_pow2(p < 2 ? 2 : p);
    size_t bytes = (sort_partial_bytes(n_pad) + 255) & ~(size_t)255;
    if (sort_two_level(n_pad)) bytes += (size_t)n_pad * sizeof(uint64_t);
    return bytes;
}

hipError_t launch_sort(hipStream_t st, const float *vin, const float *sin, const float *fin,
                       float *vout, float *sout, float *fout, uint64_t *keys, void *scratch, uint32_t p,
                       uint32_t d, uint32_t first_row, const SortExchange *exchange)
{
    const SortExchange ex = exchange ? *exchange : SortExchange{};
    const uint32_t n_pad = next_pow2(p < 2 ? 2 : p);
    if (n_pad <= kSortSmall) { // one launch
        switch ((n_pad + kWave - 1) / kWave) {
        case 1: k_sort_small<1><<<1, 1 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, first_row, ex); break;
        case 2: k_sort_small<2><<<1, 2 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, first_row, ex); break;
        case 4: k_sort_small<4><<<1, 4 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, first_row, ex); break;
        case 8: k_sort_small<8><<<1, 8 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, first_row, ex); break;
        default: k_sort_small<16><<<1, 16 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, first_row, ex); break;
        }
        return hipGetLastError();
    }
    uint32_t tile, tiles;
    sort_plan(n_pad, tile, tiles);
    uint32_t threads = tile / 2;
    threads = threads < 64 ? 64 : threads > (uint32_t)kSortThreads ? (uint32_t)kSortThreads : threads;
    const bool two_level = sort_two_level(n_pad);
    const bool rank_merge = two_level || (tiles > 1 && tiles <= kSortMaxTiles);
    if (rank_merge && tile == 4 * kRunKeys)
        k_sort_tiles_1k<<<tiles, 256, 0, st>>>(fin, keys, p);
    else
        k_sort_tiles<<<tiles, threads, 0, st>>>(fin, keys, p, tile, rank_merge ? 0u : 1u);
    if (two_level) {
        uint16_t *partial = static_cast<uint16_t *>(scratch);
        uint64_t *merged = reinterpret_cast<uint64_t *>(static_cast<char *>(scratch) +
                                                        ((sort_partial_bytes(n_pad) + 255) & ~(size_t)255));
        // level 1: groups of 8 tiles -> sorted runs of 8192 keys; level 2: every key against every run
        k_sort_rank_pairs<kRankGroup, true><<<tiles, kRankThreads, 0, st>>>(keys, nullptr, n_pad, tile, merged);
        const uint32_t runs = n_pad / kRankLdsKeys;
        k_sort_rank_pairs<1><<<dim3(runs, runs), kRankThreads, 0, st>>>(merged, partial, n_pad, kRankLdsKeys);
        k_sort_rank_scatter<<<n_pad / 64, kRankThreads, 0, st>>>(merged, partial, vin, sin, fin, vout, sout, fout,
                                                               n_pad, runs, p, d, first_row, ex);
        return hipGetLastError();
    }
    if (rank_merge) {
        uint16_t *partial = static_cast<uint16_t *>(scratch);
        const uint32_t group = rank_group(tile, tiles), groups = tiles / group;
        switch (group) {
        case 8: k_sort_rank_pairs<8><<<dim3(tiles, groups), kRankThreads, 0, st>>>(keys, partial, n_pad, tile); break;
        case 4: k_sort_rank_pairs<4><<<dim3(tiles, groups), kRankThreads, 0, st>>>(keys, partial, n_pad, tile); break;
        case 2: k_sort_rank_pairs<2><<<dim3(tiles, groups), kRankThreads, 0, st>>>(keys, partial, n_pad, tile); break;
        default: k_sort_rank_pairs<1><<<dim3(tiles, groups), kRankThreads, 0, st>>>(keys, partial, n_pad, tile); break;
        }
        k_sort_rank_scatter<<<n_pad / 64, kRankThreads, 0, st>>>(keys, partial, vin, sin, fin, vout, sout, fout,
                                                               n_pad, groups, p, d, first_row, ex);
        return hipGetLastError();
    }
    for (uint32_t k = tile << 1; k <= n_pad && k != 0; k <<= 1) {
        for (uint32_t j = k >> 1; j >= tile; j >>= 1)
            k_sort_global_step<<<grid_for(n_pad / 2, 256), 256, 0, st>>>(keys, n_pad, k, j);
        k_sort_tile_merge<<<tiles, threads, 0, st>>>(keys, k, tile);
    }
    k_sort_gather<<<grid_for((uint64_t)p * (2 * d + 1), 256), 256, 0, st>>>(keys, vin, sin, fin, vout, sout,
                                                                            fout, p, d, first_row, ex);
    return hipGetLastError();
}

// keys buffer: n_pad 64-bit keys (full sort) or n_pad fitness-bit words + n_pad indices (selection),
// followed by the selection's per-tile samples
// The selection's key arrays: the population padded to a power of two and to at least kSelMinTiles tiles (the rank kernel
// holds one sample per lane and more: 16 tiles x 4 samples); a population of 2048 ... 8192 simply has tiles of nothing but
// padding keys behind its own (they sort last, stage one quantum each and move nothing)
static uint32_t sel_pad(uint32_t p)
{
    const uint32_t n_pad = next_pow2(p < 2 ? 2 : p);
    return n_pad < kSelMinTiles * kSelTile ? kSelMinTiles * kSelTile : n_pad;
}

size_t sort_keys_bytes(uint32_t p)
{
    const uint32_t n_pad = p > kSortSmall ? sel_pad(p) : next_pow2(p < 2 ? 2 : p);
    return (size_t)n_pad * sizeof(uint64_t) + (size_t)2 * kSelMaxTiles * kSelSamples * sizeof(uint32_t);
}

// The selection applies to every population that does not fit k_sort_small's one launch (P > 1024; round 3: it used to start at
// 8192, the three launches of the tile sort below that took 20-23 us where the selection's two take 15) while at most half of
// the rows are wanted (beyond that nearly everything would be staged and the full sort is the better plan).  Up to 64 tiles
// (P <= 65536) the rank kernel works on the 1024-key tiles; at 128 tiles (P <= 131072) they are first merged four by four
// (k_sel_merge4), which quarters its work; larger populations take the two-level full sort.
constexpr uint32_t kSelDirectTiles = 64, kSelMergedTiles = 128;
bool select_applies(uint32_t p, uint32_t need)
{
    const uint32_t tiles = sel_pad(p) / kSelTile;
    return p > kSortSmall && tiles <= kSelMergedTiles && need >= 1 && (uint64_t)need * 2 <= p;
}

// scratch of the merged plan: the 4096-key tiles (bits, indices) and their samples
size_t select_scratch_bytes(uint32_t p)
{
    const uint32_t n_pad = sel_pad(p);
    return (size_t)n_pad * 2 * sizeof(uint32_t) + (size_t)2 * kSelMaxTiles * kSelSamples * sizeof(uint32_t);
}

hipError_t launch_select(hipStream_t st, const float *vin, const float *sin, const float *fin, float *vout,
                         float *sout, float *fout, uint64_t *keys, void *scratch, uint32_t p, uint32_t d, uint32_t need,
                         uint32_t num_cus, const SortExchange *exchange)
{
    if (!select_applies(p, need)) return hipErrorInvalidValue;
    const SortExchange ex = exchange ? *exchange : SortExchange{};
    const uint32_t n_pad = sel_pad(p);
    const uint32_t tiles = n_pad / kSelTile;
    uint32_t *kbits = reinterpret_cast<uint32_t *>(keys), *kidx = kbits + n_pad, *samples = kidx + n_pad;
    // (split while the parts still find CUs of their own; the 128 tiles of P = 131072 stay whole)
    if (SOTS_SEL_SPLIT > 1 && tiles * SOTS_SEL_SPLIT <= (num_cus ? num_cus : 256))
        k_sel_tiles<SOTS_SEL_SPLIT><<<tiles * SOTS_SEL_SPLIT, kSelTile, 0, st>>>(fin, kbits, kidx, samples, p, tiles);
    else k_sel_tiles<1><<<tiles, kSelTile, 0, st>>>(fin, kbits, kidx, samples, p, tiles);
    // one workgroup per CU (the staging buffer takes the LDS); more only when a share of the staged
    // positions would exceed the per-workgroup key store
    uint32_t grid = num_cus ? num_cus : 256;
    const uint32_t min_grid = (tiles * kSelTile + kSelMaxOwn - 1) / kSelMaxOwn;
    if (grid < min_grid) grid = min_grid;
    // lanes per key x 8 search chains = the tiles one pass stages: 64 / 32 / 16 tiles of 1024 keys, <= 20 big tiles
    // at most 8 real tiles (P <= 8192): they are staged whole (32 KiB), the padding tiles not at all
    const uint32_t real_tiles = (p + kSelTile - 1) / kSelTile, whole = real_tiles <= 8 ? real_tiles : 0u;
#define SOTS_SEL(R, T, Q, L, KB, KI, SM, NT) \
    k_sel_rank_scatter<R, T, Q, L><<<grid, kSelThreads, 0, st>>>(KB, KI, SM, vin, sin, fin, vout, sout, fout, NT, need, p, d, ex, whole)
    if (tiles <= kSelDirectTiles) {
        switch (tiles * kSelSamples / kWave) {
        case 1: SOTS_SEL(1, kSelTile, kSelQuantum, 2, kbits, kidx, samples, tiles); break;
        case 2: SOTS_SEL(2, kSelTile, kSelQuantum, 4, kbits, kidx, samples, tiles); break;
        case 4: SOTS_SEL(4, kSelTile, kSelQuantum, 8, kbits, kidx, samples, tiles); break;
        default: return hipErrorInvalidValue;
        }
    } else {
        uint32_t *bbits = static_cast<uint32_t *>(scratch), *bidx = bbits + n_pad, *bsamples = bidx + n_pad;
        const uint32_t big = tiles / 4;
        k_sel_merge4<<<big, kSelTile, 0, st>>>(kbits, kidx, bbits, bidx, bsamples);
        switch (big * kSelBigSamples / kWave) {
        case 4: SOTS_SEL(4, kSelBigTile, kSelBigQuantum, 4, bbits, bidx, bsamples, big); break;
        default: return hipErrorInvalidValue;
        }
    }
#undef SOTS_SEL
    return hipGetLastError();
}

// ---- the one-launch selection between stored splitters (k_sel_splitters) ----
// a slot: one splitter per workgroup, one workgroup per CU
uint32_t select_splitter_count(uint32_t num_cus)
{
    const uint32_t b = num_cus ? num_cus : 256;
    return b > kSplMaxBuckets ? kSplMaxBuckets : b < 2 ? 2 : b;
}
size_t select_splitter_slot_bytes() { return (size_t)kSplMaxBuckets * sizeof(uint64_t); }
// positions q * step of one generation's order are the next one's splitters: the old order up to 1.25 * need.  While a
// run improves, the next generation puts 1.3 ... 4 times as many keys below an old key as the old generation did
// (profiles/r06_experiments.md); a converged population whose fitness values all tie puts exactly as many.  The cut
// of the next generation must fall inside the slot: behind the last splitter one workgroup owns all the rest.
static uint32_t select_splitter_step(uint32_t need, uint32_t buckets)
{
    return (uint32_t)(((uint64_t)need * 5 / 4 + buckets - 2) / (buckets - 1)); // >= 1 (need >= 1); (buckets - 1) * step < P as need <= P / 2
}

hipError_t launch_select_splitters(hipStream_t st, const float *vin, const float *sin, const float *fin, float *vout,
                                   float *sout, float *fout, uint64_t *keys, const uint64_t *spl_in, uint64_t *spl_out,
                                   uint32_t p, uint32_t d, uint32_t need, uint32_t num_cus, const SortExchange *exchange,
                                   const SelLists *lists)
{
    if (!select_applies(p, need)) return hipErrorInvalidValue;
    const SortExchange ex = exchange ? *exchange : SortExchange{};
    const uint32_t buckets = select_splitter_count(num_cus);
    if (lists && (buckets > kSelListMaxBuckets || lists->buckets != buckets || lists->slot != spl_in || !lists->cnt || !lists->cnt_other || !lists->lists)) return hipErrorInvalidValue;
    // bit 0: the fitness can be read 16 bytes per lane; bit 1: so can rows of four genes
    const uintptr_t row_bits = reinterpret_cast<uintptr_t>(vin) | reinterpret_cast<uintptr_t>(sin) | reinterpret_cast<uintptr_t>(vout) | reinterpret_cast<uintptr_t>(sout);
    const uint32_t vec = ((reinterpret_cast<uintptr_t>(fin) & 15u) == 0 ? 1u : 0u) | ((row_bits & 15u) == 0 ? 2u : 0u);
    k_sel_splitters<<<buckets, kSplThreads, 0, st>>>(vin, sin, fin, vout, sout, fout, spl_in, spl_out, keys, p, need,
                                                     select_splitter_step(need, buckets), d, ex, vec, lists ? *lists : SelLists{});
    return hipGetLastError();
}

// ---- list mode: who files the keys ----
bool select_lists_apply(uint32_t p, uint32_t log2n, uint32_t num_cus)
{
    return fft_wide(p, log2n, num_cus) && select_splitter_count(num_cus) <= kBktMaxBuckets;
}
size_t select_lists_bytes(uint32_t num_cus) { return (size_t)select_splitter_count(num_cus) * kSelListCap * sizeof(uint64_t); }
size_t select_counters_bytes() { return (size_t)kSelListMaxBuckets * kSelListShards * sizeof(uint32_t); }

} // namespace sots

#include "kernels/bucket_fitness.h"

namespace sots {

hipError_t launch_bucket_fitness(hipStream_t st, const float *fitness, uint32_t p, const SelLists &lists)
{
    if (lists.buckets < 2 || lists.buckets > kBktMaxBuckets || !lists.slot || !lists.cnt || !lists.lists) return hipErrorInvalidValue;
    const uint32_t grid = (p + kBktThreads - 1) / kBktThreads;
    if (bkt_two_level(p)) k_bucket_fitness<kBktTwoLevel><<<grid, kBktThreads, 0, st>>>(fitness, p, lists);
    else k_bucket_fitness<kBktFlat><<<grid, kBktThreads, 0, st>>>(fitness, p, lists);
    return hipGetLastError();
}

hipError_t launch_select_seed(hipStream_t st, const float *fsorted, uint64_t *spl_out, uint32_t need, uint32_t num_cus)
{
    const uint32_t buckets = select_splitter_count(num_cus);
    k_sel_seed<<<1, kSplMaxBuckets, 0, st>>>(fsorted, spl_out, need, select_splitter_step(need, buckets), buckets);
    return hipGetLastError();
}

hipError_t launch_pack_rows(hipStream_t st, const float *values, const float *steps, const float *fitness,
                            float *rows, uint32_t first_row, uint32_t n_rows, uint32_t d)
{
    if (n_rows == 0) return hipSuccess;
    k_pack_rows<<<grid_for((uint64_t)n_rows * (2 * d + 1), 256), 256, 0, st>>>(values, steps, fitness, rows,
                                                                               first_row, n_rows, d);
    return hipGetLastError();
}

hipError_t launch_unpack_rows(hipStream_t st, float *values, float *steps, float *fitness,
                              const float *rows, uint32_t first_row, uint32_t n_rows, uint32_t d,
                              uint32_t skip_first, uint32_t skip_count)
{
    if (n_rows == 0) return hipSuccess;
    k_unpack_rows<<<grid_for((uint64_t)n_rows * (2 * d + 1), 256), 256, 0, st>>>(values, steps, fitness, rows,
                                                                                 first_row, n_rows, d, skip_first,
                                                                                 skip_count);
    return hipGetLastError();
}

// ---- chunks in flight ----------------------------------------------------------------
hipError_t launch_init_population_seg(hipStream_t st, float *values, float *steps, float *fitness, const PopDims &pd,
                                      uint32_t first_chunk, uint32_t chunks)
{
    k_init_population_seg<<<grid_for((uint64_t)chunks * pd.p * pd.d, 256), 256, 0, st>>>(values, steps, fitness, pd, first_chunk, chunks);
    return hipGetLastError();
}

hipError_t launch_recombine_mutate_seg(hipStream_t st, const float *vin, const float *sin, float *vout, float *sout,
                                       const PopDims &pd, const MutateConsts &mc, uint32_t generation, uint32_t chunks)
{
    k_recombine_mutate_seg<<<grid_for((uint64_t)chunks * pd.p * pd.d, 256), 256, 0, st>>>(vin, sin, vout, sout, pd, mc, generation, chunks);
    return hipGetLastError();
}

size_t seg_target_stride(uint32_t log2n)
{
    const size_t bins = (1u << log2n) / 2u;
    if (!x_from(log2n)) return bins;
    return for_log2n(XSizes{}, log2n, bins, [](auto l) { return (size_t)x_seg_stride<decltype(l)::value>(); });
}

size_t seg_target_bytes(uint32_t log2n, uint32_t chunks)
{
    return (kSegHead + (size_t)chunks * seg_target_stride(log2n)) * sizeof(float);
}

hipError_t launch_seg_targets(hipStream_t st, float *image, const float *targets, uint32_t log2n, uint32_t chunks)
{
    float *tables = image + kSegHead;
    if (!x_from(log2n))
        return hipMemcpyAsync(tables, targets, (size_t)chunks * ((1u << log2n) / 2u) * sizeof(float), hipMemcpyDeviceToDevice, st);
    const uint64_t work = (uint64_t)chunks * (1u << log2n) / 2u;
    return for_log2n(XSizes{}, log2n, hipErrorInvalidValue, [&](auto l) {
        k_x_seg_targets<decltype(l)::value><<<grid_for(work, 256), 256, 0, st>>>(tables, targets, chunks);
        return hipGetLastError();
    });
}

// The weight table of the fused kernels: u[N/2] laid out as ONE chunk's target table (plain bins for k_fft and k_fft_big,
// the per-(lane, register) table for k_fft_x), so the weighted kernels read u wherever they read the target
size_t weight_image_bytes(uint32_t log2n) { return seg_target_bytes(log2n, 1); }
hipError_t launch_weight_image(hipStream_t st, float *image, const float *u, uint32_t log2n)
{
    const hipError_t e = hipMemsetAsync(image, 0, weight_image_bytes(log2n), st); // (the padding entries are never read; they are defined all the same)
    if (e != hipSuccess) return e;
    return launch_seg_targets(st, image, u, log2n, 1);
}

// launch_fft_fitness with a window, every row against its chunk's target: each kernel's SEG instantiation
hipError_t launch_fft_fitness_seg(hipStream_t st, const float *audio, const float *window, const float *seg_image, float *fitness,
                                  const float2 *twiddle, uint32_t p, uint32_t log2n, uint32_t pitch, float inv_n, float inv_wf,
                                  uint32_t num_cus, OccCache *oc, const Objective &obj)
{
    return launch_fused_objective<true>(st, audio, window, seg_image, fitness, twiddle, p, log2n, pitch, inv_n, inv_wf, num_cus, oc, nullptr, obj);
}

hipError_t launch_sort_seg(hipStream_t st, const float *vin, const float *sin, const float *fin, float *vout, float *sout,
                           float *fout, uint32_t p, uint32_t d, uint32_t chunks)
{
    const uint32_t n_pad = next_pow2(p < 2 ? 2 : p);
    if (n_pad > kSortSmall) return hipErrorInvalidValue;
    const SortExchange ex{};
    switch ((n_pad + kWave - 1) / kWave) {
    case 1: k_sort_small<1, true><<<chunks, 1 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, 0, ex); break;
    case 2: k_sort_small<2, true><<<chunks, 2 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, 0, ex); break;
    case 4: k_sort_small<4, true><<<chunks, 4 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, 0, ex); break;
    case 8: k_sort_small<8, true><<<chunks, 8 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, 0, ex); break;
    default: k_sort_small<16, true><<<chunks, 16 * kWave, 0, st>>>(vin, sin, fin, vout, sout, fout, p, d, 0, ex); break;
    }
    return hipGetLastError();
}

} // namespace sots

#include "kernels/track.h"
#include "kernels/queue.h"

namespace sots {

hipError_t launch_recombine_mutate_queue(hipStream_t st, const float *vin, const float *sin, float *vout, float *sout, const PopDims &pd,
                                         const MutateConsts &mc, const uint32_t *slot_table, uint32_t slots)
{
    k_recombine_mutate_queue<<<grid_for((uint64_t)slots * pd.p * pd.d, 256), 256, 0, st>>>(vin, sin, vout, sout, pd, mc, slot_table, slots);
    return hipGetLastError();
}

uint32_t queue_x_log2n(uint32_t log2n) { return x_from(log2n) && log2n != 10 ? log2n : 0u; }

hipError_t launch_queue_turnover(hipStream_t st, float *values, float *steps, float *fitness, const PopDims &pd, uint32_t *meta,
                                 float *rows, const QueueArgs &q, uint32_t global_generation, uint32_t slots)
{
    if (slots == 0 || pd.d == 0 || pd.d > SOTS_MAX_DIMS || q.num_chunks == 0 || q.max_generations == 0) return hipErrorInvalidValue;
    if (q.carry_rows) {
        // (the kernel trusts these: rows 0..R-1 lie inside the slot's population, and the segment arithmetic neither divides by 0 nor wraps)
        if (q.carry_rows > pd.p || q.segment_chunks == 0 || q.num_segments != (q.num_chunks - 1u) / q.segment_chunks + 1u) return hipErrorInvalidValue;
        k_queue_turnover<true><<<slots, 256, 0, st>>>(values, steps, fitness, pd, meta, rows, q, global_generation);
    } else {
        k_queue_turnover<false><<<slots, 256, 0, st>>>(values, steps, fitness, pd, meta, rows, q, global_generation);
    }
    return hipGetLastError();
}

hipError_t launch_track_clear(hipStream_t st, uint32_t *meta, float *rows, uint32_t chunks)
{
    k_track_clear<<<grid_for((uint64_t)chunks * (2u + kTrackRowFloats), 256), 256, 0, st>>>(meta, rows, chunks);
    return hipGetLastError();
}

hipError_t launch_track(hipStream_t st, const float *values, const float *steps, const float *fitness, uint32_t p, uint32_t d,
                        uint32_t parents, uint32_t generation, uint32_t chunks, uint32_t *meta, float *rows, float *hist,
                        uint32_t capacity, uint32_t slot)
{
    if (chunks == 0 || d == 0 || d > SOTS_MAX_DIMS || parents == 0 || parents > p) return hipErrorInvalidValue;
    if (slot != kTrackNoSlot && (!hist || slot >= capacity)) return hipErrorInvalidValue;
    k_track<<<chunks, track_threads(parents, d), 0, st>>>(values, steps, fitness, p, d, parents, generation, meta, rows, hist, capacity, slot);
    return hipGetLastError();
}

} // namespace sots

#if defined(SOTS_STAMP) || defined(SOTS_STAMP_ENDS)
extern "C" int sots_debug_stamps(unsigned long long *host, size_t n)
{
    if (n > 2 * 16384) n = 2 * 16384;
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(sots::g_stamps), n * sizeof(unsigned long long));
}
extern "C" int sots_debug_clear_stamps()
{
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(sots::g_stamps)) != hipSuccess) return -1;
    return (int)hipMemset(p, 0, sizeof(unsigned long long) * 2 * 16384);
}
#endif
