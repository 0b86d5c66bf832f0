// Evolutionary_Strategy_HIP.hpp -- the MI355X backend: a drop-in for
// Evolutionary_Strategy_{OpenCL,CUDA,Vulkan} behind the Evolutionary_Strategy base class.
//
// All device work goes through the C-ABI of include/sots_hip.h (libsots_hip.so); this class
// is the thin C++ host side the reference's main.cpp drives:
//   construct from *_Arguments           (Evolutionary_Strategy_OpenCL.hpp:25-38,122-137)
//   parameterMatchAudio(audio, length)   (:572-610)  chunk loop, timers, CSV
//   readPopulationData(...)              (:417-430)
//   printBest()                          (:613-631)
// Stage timers keep the reference's names (:117) and feed the Benchmarker through
// addTimer(name, ms) with hipEvent-measured durations, like the Vulkan backend feeds its
// timestamp queries (Evolutionary_Strategy_Vulkan.hpp:1169-1210); with chunksInFlight > 1 (chunks matched in
// batches, sots_batch) only the "Total Audio Analysis Time" row is produced, no per-stage rows.  Errors, which the
// reference prints and ignores, throw std::runtime_error here (main.cpp:282 catches it).
#ifndef SOTS_EVOLUTIONARY_STRATEGY_HIP_HPP
#define SOTS_EVOLUTIONARY_STRATEGY_HIP_HPP

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sots_hip.h"
#include "Benchmarker.hpp"
#include "Evolutionary_Strategy.hpp"
#include "Match_track.hpp"
#include "Objective_weights.hpp"

struct Evolutionary_Strategy_HIP_Arguments
{
    // Generic Evolutionary Strategy arguments
    Evolutionary_Strategy_Arguments es_args;

    // HIP details (mirror of the OpenCL block)
    uint32_t workgroupX = 32; // recombination block, ocl_program.cl WRKGRPSIZE
    uint32_t workgroupY = 1;
    uint32_t workgroupZ = 1;
    uint32_t workgroupSize = workgroupX * workgroupY * workgroupZ;

    int32_t deviceOrdinal = 0;        // replaces deviceType / vendor-id matching
    uint64_t seed = 0x5EED0001ull;    // replaces the wall-clock seed
    uint32_t gidBase = 0;             // island offset of individual 0
    int32_t synthKind = -1;           // -1: derive from numDimensions (4, 6, 8, 12)
    // The operator-graph voice (type.HIP.synth "graph" with type.HIP.voiceGraph; sots_create_graph): with
    // synthKind SOTS_SYNTH_GRAPH the topology, numDimensions = 2 x num_operators.  One device; matchPath, renderMatch
    // (overlap-add, or renderMode 3 and 4), matchReport, chunksInFlight and chunkQueue work with it; renderMode 1 and 2 with renderMatch and
    // deviceKernelArithmetic do not: the constructor throws - before any device work - and a malformed graph is refused there
    // with the library's own text.
    sots_voice_graph voiceGraph{};
    // ... and its operators' waveforms (type.HIP.voiceWaveforms; sots_set_voice_waveforms): SOTS_WAVE_* per
    // operator, or empty: all sine.  Only with the graph voice: the constructor throws before any device work otherwise.
    std::vector<uint32_t> voiceWaveforms;
    // ... and their feedback indices (type.HIP.voiceFeedback; sots_set_voice_feedback): one number in [0, 2]
    // per operator, or empty: none.  Only with the graph voice, as the waveforms.
    std::vector<float> voiceFeedback;
    // ... or, for the operators in this mask, a gene of the individual (type.HIP.voiceFeedbackGenes; sots_create_graph_genes,
    // DESIGN.md 4.18): numDimensions = 2 x num_operators + the set bits, the genes' ranges behind the others.  Only with the
    // graph voice and not with renderMode 3 to 6 (7 and 8 render it): the constructor throws before any device work; the
    // library refuses the rest.
    uint32_t voiceFeedbackGenes = 0;
    // ... and which synthesis kernel the graph voice runs (type.HIP.graphSynthForm; sots_set_graph_synth_form, DESIGN.md
    // 4.20): enum sots_graph_synth_form, the same audio bit for bit.  Only with the graph voice, as the waveforms.
    uint32_t graphSynthForm = 0;
    bool fusedGenerations = true;     // executeAllGenerations uses the fused kernel loop
    // general.isBenchmarking (parameters.json:7, main.cpp:85).  true: every launch is bracketed by a
    // hipEvent pair and lands in the CSV under the reference's stage names (an event pair costs
    // about 3.5 us per kernel boundary: 170 vs 144 us per generation at pop = 65536).  false: the
    // un-instrumented loop - no events, one wall-clock "Total Audio Analysis Time" row and a
    // candidates-per-second line ("plus an un-instrumented mode").
    bool benchmarkStages = true;
    // true: sortPopulation orders all P rows every generation as the reference does; false: each generation places
    // the rows the next recombination reads and the rest of the order is produced when it is read (same results)
    bool fullSortEveryGeneration = false;
    // false (default): the synthesis arithmetic of the reference's CPU path (fp32 sample-rate ratio, Evolutionary_Strategy.hpp:203);
    // true: that of its OpenCL kernels (double ratio, fused multiply-adds, 3-op offset params[4]: ocl_program.cl:280-443) -
    // bit-identical audio to those kernels, through one plain kernel (enum sots_synth_arith); not for the 4-op voice
    bool deviceKernelArithmetic = false;
    // Island model inside this object (type.HIP.{numDevices,numElites,migrationInterval} in parameters.json;
    // the reference picks exactly one device, ...OpenCL.hpp:194-226).  es_args.pop describes ONE island; with
    // numDevices > 1 the object owns one island per device (devices[i], default deviceOrdinal + i), PRNG ids
    // gidBase + i * populationLength, and every migrationInterval generations the islands' best numElites
    // rows are all-gathered over RCCL and replace the tail of the other islands' parents.  Results are read
    // from the island holding the best individual; stage timers are island 0's.
    uint32_t numDevices = 1;
    std::vector<int32_t> devices;     // empty: deviceOrdinal, deviceOrdinal + 1, ...
    uint32_t numElites = 16;
    uint32_t migrationInterval = 1;
    bool overlapMigration = false;    // the all-gather runs underneath the next generation, rows arrive one exchange later
    // Chunks in flight (type.HIP.chunksInFlight): with more than 1, a single device and populationLength <= 1024,
    // parameterMatchAudio matches that many chunks at once (sots_batch: every chunk against its own target, the launches
    // of one population per generation) - same results as the chunk-by-chunk loop.  In that mode the CSV gets only the
    // "Total Audio Analysis Time" row, no per-stage rows.  Otherwise (numDevices > 1, P > 1024) the chunk-by-chunk loop.
    uint32_t chunksInFlight = 1;
    // Run record (type.HIP.{returnBestEver,historyEvery,historyPath,targetFitness,stallGenerations,stopCheckInterval};
    // extends parameterMatchAudio and printBest, Evolutionary_Strategy_OpenCL.hpp:572-631, which report row 0 of the last
    // of a fixed number of generations).  The strategy is not elitist, so that row can be worse than one held earlier.
    // All off by default; single device only.
    //   returnBestEver   : recordBest(), bestParametersPerChunk() and sots_match's final rendering use the best individual
    //                      any generation of the chunk produced (kept on the device, sots_track)
    //   historyEvery > 0 : a record of the parent rows every that many generations; with historyPath, written as CSV
    //                      (chunk,generation,best,best_ever,parent_mean,parent_worst,step_0..step_{D-1}), one row per record
    //   targetFitness >= 0 / stallGenerations > 0 : a chunk stops before numGenerations once its best-ever fitness is <= the
    //                      target, or has not improved for stallGenerations generations; looked at every stopCheckInterval
    //                      generations (sots_execute_until).  Chunks in flight advance together until every chunk of the
    //                      batch has stopped; each chunk's result is taken at ITS stopping boundary, so it does not depend
    //                      on chunksInFlight (its history goes on to the batch's last boundary).
    // Chunk queue (type.HIP.chunkQueue; sots_batch_queue_run): with chunksInFlight > 1 and no historyPath, parameterMatchAudio
    // sends ALL its chunks through the chunksInFlight slots of one batch - a chunk whose stop rule holds (or that has run
    // numGenerations) is retired on the device and its slot starts the next chunk at once, instead of idling until the slowest
    // chunk of its batch is done.  Same per-chunk results, same lines printed.  With a historyPath (the slots keep no history
    // rings) today's batch-by-batch path runs.  Off by default: nothing changes.
    bool chunkQueue = false;
    // Carried rows (type.HIP.{carryRows,segmentChunks}; sots_batch_queue_set_carry), chunk queue only: the
    // chunks are cut into segments of segmentChunks consecutive chunks, and inside a segment a chunk starts from its
    // predecessor's best-ever individual (row 0) and rows 1..carryRows-1 beside fresh rows, so that neighbouring rows of the
    // parameter track describe one voice.  carryRows 0 (default): off, nothing changes.  segmentChunks 0: ceil(chunks /
    // chunksInFlight), one segment per slot.  Meant for survivors >= 1.  Where the queue does not run (chunksInFlight 1,
    // numDevices > 1, populationLength > 1024) parameterMatchAudio throws rather than match without carrying.
    uint32_t carryRows = 0;
    uint32_t segmentChunks = 0;
    // Analysis on the device (type.HIP.{deviceAnalysis,matchReport}; sots_batch_set_analysis).
    //   deviceAnalysis : the chunks in flight (batched and queued alike) get their target spectra from ONE upload of the audio
    //                    per batch - the library's fp32 transform on the device - instead of Objective::calculateFFT chunk by
    //                    chunk on the host.  The targets are then not the host's bits (fp32 against fp64), so neither are the
    //                    matches: off by default.  Where matching would go chunk by chunk (chunksInFlight <= 1, numDevices > 1,
    //                    populationLength > 1024) the constructor throws - before any device work - rather than fall back.
    //   matchReport    : sots_match scores the rendered match against the stored targets, chunk by chunk (scoreAgainstTargets()
    //                    below), and writes chunk,fitness,rendered_fitness there.  Needs renderMatch and the chunk queue (it
    //                    keeps the targets); otherwise the constructor throws the same way.
    bool deviceAnalysis = false;
    std::string matchReport = "";
    // Elitist survival (type.HIP.survivors; sots_set_survivors): rows 0..survivors-1 of the sorted population pass through
    // recombination and mutation unchanged and are evaluated again with the offspring.  0 (default) is the reference's
    // strategy; at most numParents, above that the constructor / parameterMatchAudio throws with the library's text.
    // Applied to the context, to every island of a group and to the chunks in flight (batched and queued alike).
    uint32_t survivors = 0;
    // The spectral objective (type.HIP.objective, type.HIP.objectiveFloor; sots_set_objective): SOTS_OBJECTIVE_MAGNITUDE, the
    // reference's sum of squared magnitude differences (default), or SOTS_OBJECTIVE_LOG_MAGNITUDE, the sum over the same
    // bins of (ln(m + objectiveFloor) - ln(t + objectiveFloor))^2 with 1e-30 <= objectiveFloor <= 1.  Applied to the context,
    // to every island of a group and to the chunks in flight (batched and queued alike).  Every fitness printed, the
    // history's columns and targetFitness are in the units of the objective in force.  objectiveGiven: sots_match
    // names the objective in its output (one line) only when parameters.json named it.
    uint32_t objective = SOTS_OBJECTIVE_MAGNITUDE;
    float objectiveFloor = 0.0f;
    bool objectiveGiven = false;
    // Per-bin weights of the objective (type.HIP.objectiveWeights; sots_set_objective_weights, Objective_weights.hpp): a
    // band in Hz, the A-curve or a table of N/2 numbers; the fitness is then sum_k w_k e_k^2 over the bins, and every
    // fitness printed, the history's columns and targetFitness are in the units of that weighted sum.  The table is made
    // for N and the class's sampleRate in the constructor, which throws - before any device work - where it cannot be.
    // Applied to the context, to every island of a group and to the chunks in flight (batched and queued alike).
    // sots_match names the weighting in its output (one line) only when parameters.json named it.
    Objective_Weights_Spec objectiveWeights;
    // Analysis at a hop and the rendering of the whole match (type.HIP.{hopSize,renderMatch,matchPath}).
    //   hopSize     : samples between chunk starts; 0 (default) = the audio length N, the reference's chunking.  Otherwise
    //                 ceil(N / 64) <= hopSize <= N, need not divide N; the constructor throws - before any device work - where
    //                 it is not.  parameterMatchAudio then matches chunk i = samples [i hopSize, i hopSize + N), (L - N) / hopSize
    //                 + 1 of them, in all its paths (chunk by chunk, in flight, queued).
    //   renderMatch : sots_match writes the overlap-add rendering of every chunk's match (renderMatch() below) to
    //                 outputAudioPath instead of 2^14 samples of the last chunk's
    //   renderMode  : which renderer renderMatch() uses: 0 = overlap-add (the default), 1 = phase-continuous
    //                 (sots_render_continuous: one voice whose oscillators never restart, parameters held from chunk centre to
    //                 chunk centre), 2 = phase-continuous with the parameters interpolated between the centres.  Takes effect
    //                 only with renderMatch; 1 and 2 are not available with deviceKernelArithmetic.  3 and 4 are 1 and 2 for the
    //                 operator-graph voice (sots_render_graph_continuous) and need it.  5 and 6 are 3 and 4 for a
    //                 graph voice with feedback indices (sots_render_graph_feedback).  7 and 8 are 5 and 6 for a
    //                 graph voice whose feedback indices may be genes (sots_render_graph_genes).
    //   matchPath   : sots_match writes the parameter track there, one CSV row per chunk (Match_track.hpp)
    uint32_t hopSize = 0;
    bool renderMatch = false;
    uint32_t renderMode = 0;
    std::string matchPath = "";
    bool returnBestEver = false;
    uint32_t historyEvery = 0;
    std::string historyPath = "";
    float targetFitness = -1.0f;
    uint32_t stallGenerations = 0;
    uint32_t stopCheckInterval = 32;
    bool verbose = true;
    std::string logDirectory = "";    // where hiplog(...).csv goes ("" = cwd)
};

class Evolutionary_Strategy_HIP : public Evolutionary_Strategy
{
private:
    static const uint8_t numKernels_ = 9;
    enum kernelNames_ { initPopulation = 0, recombinePopulation, mutatePopulation, synthesisePopulation, applyWindowPopulation, hipFFT, fitnessPopulation, sortPopulation, rotatePopulation };
    std::array<std::string, numKernels_> kernelNames_;

    sots_ctx *ctx_ = nullptr;       // the context results and timers are read from (island 0 / the best island of a group)
    sots_group *group_ = nullptr;   // owns the islands when numDevices > 1
    sots_batch *batch_ = nullptr;   // chunks in flight (args_.chunksInFlight > 1), made by the first batched parameterMatchAudio
    sots_config cfg_{};
    Evolutionary_Strategy_HIP_Arguments args_;

    uint32_t numChunks_ = 0;
    uint32_t chunkSize_ = 0;
    uint32_t hop_ = 0;              // samples between chunk starts: args_.hopSize, or the audio length
    uint32_t targetAudioLength = 0;
    std::vector<float> targetFFT_;
    std::vector<float> objectiveWeights_;       // the table of args_.objectiveWeights for this N; empty: no weights
    std::vector<std::vector<float>> bestPerChunk_;
    std::vector<float> bestFitnessPerChunk_;
    std::vector<uint32_t> generationsPerChunk_; // generations each chunk's result was taken after
    uint64_t generationsRun_ = 0;               // generations really run, over all chunks, by the last parameterMatchAudio
    uint32_t lastRun_ = 0;                      // ... by the last executeAllGenerations
    sots_stop_rule rule_{};
    FILE *historyFile_ = nullptr;
    std::vector<float> launchScratch_;
    uint32_t bestIsland_ = 0;
    double candidatesPerSecond_ = 0.0;

    Benchmarker hipBenchmarker_;

    static int kindFromDims(uint32_t d)
    {
        switch (d) {
        case 4: return SOTS_SYNTH_2OP;
        case 6: return SOTS_SYNTH_3OP_SERIES;
        case 8: return SOTS_SYNTH_4OP_SERIES;
        case 12: return SOTS_SYNTH_TRIPLE_PAR;
        default: return -1;
        }
    }
    // the chunks in flight: a batch of the context's configuration (and graph)
    void createBatch()
    {
        const bool graphVoice = cfg_.synth_kind == SOTS_SYNTH_GRAPH;
        const bool genes = graphVoice && args_.voiceFeedbackGenes != 0u;
        const int rc = genes        ? sots_batch_create_graph_genes(&cfg_, &args_.voiceGraph, args_.voiceFeedbackGenes, args_.chunksInFlight, &batch_)
                       : graphVoice ? sots_batch_create_graph(&cfg_, &args_.voiceGraph, args_.chunksInFlight, &batch_)
                                    : sots_batch_create(&cfg_, args_.chunksInFlight, &batch_);
        if (rc != SOTS_OK)
            throw std::runtime_error(std::string("Evolutionary_Strategy_HIP: ") +
                                     (genes ? "sots_batch_create_graph_genes: " : graphVoice ? "sots_batch_create_graph: " : "sots_batch_create: ") +
                                     sots_batch_last_error(nullptr));
        if (!args_.voiceWaveforms.empty() &&
            sots_batch_set_voice_waveforms(batch_, args_.voiceWaveforms.data(), (uint32_t)args_.voiceWaveforms.size()) != SOTS_OK)
            throw std::runtime_error(std::string("Evolutionary_Strategy_HIP: sots_batch_set_voice_waveforms: ") + sots_batch_last_error(batch_));
        if (!args_.voiceFeedback.empty() &&
            sots_batch_set_voice_feedback(batch_, args_.voiceFeedback.data(), (uint32_t)args_.voiceFeedback.size()) != SOTS_OK)
            throw std::runtime_error(std::string("Evolutionary_Strategy_HIP: sots_batch_set_voice_feedback: ") + sots_batch_last_error(batch_));
        if (args_.graphSynthForm != 0u && sots_batch_set_graph_synth_form(batch_, args_.graphSynthForm) != SOTS_OK)
            throw std::runtime_error(std::string("Evolutionary_Strategy_HIP: sots_batch_set_graph_synth_form: ") + sots_batch_last_error(batch_));
    }
    void check(int rc, const char *what) const
    {
        if (rc != SOTS_OK)
            throw std::runtime_error(std::string("Evolutionary_Strategy_HIP: ") + what + ": " + sots_last_error(ctx_));
    }
    void checkGroup(int rc, const char *what) const
    {
        if (rc != SOTS_OK)
            throw std::runtime_error(std::string("Evolutionary_Strategy_HIP: ") + what + ": " + sots_group_last_error(group_));
    }
    // the island whose best individual is the group's best becomes the one that is read
    void selectBestIsland()
    {
        if (!group_) return;
        uint32_t island = 0;
        float fitness = 0.0f;
        checkGroup(sots_group_best(group_, &island, &fitness), "sots_group_best");
        ctx_ = sots_group_island(group_, island);
        bestIsland_ = island;
    }
    static std::string logName(const Evolutionary_Strategy_HIP_Arguments &a)
    {
        const std::string dir = a.logDirectory.empty() ? "" : a.logDirectory + "/";
        return dir + "hiplog(pop=" + std::to_string(a.es_args.pop.populationLength) + "gens=" + std::to_string(a.es_args.numGenerations) +
               "audioBlockSize=" + std::to_string(1u << a.es_args.audioLengthLog2) + ").csv";
    }
    // hipEvent durations of the launches since the last harvest -> Benchmarker, ONE addTimer per
    // launch, so that the CSV's Average/Max/Min/difference columns are per launch as in the
    // reference (Benchmarker.hpp:33-72); launches beyond the library's per-stage sample store
    // (65536 between harvests) are added as one remainder
    void harvestStage(int stage, const std::string &name)
    {
        double ms = 0.0;
        uint64_t n = 0, got = 0;
        check(sots_stage_time_ms(ctx_, stage, &ms, &n), "sots_stage_time_ms");
        if (!n) return;
        launchScratch_.resize((size_t)std::min<uint64_t>(n, 65536));
        check(sots_stage_launch_times_ms(ctx_, stage, launchScratch_.data(), launchScratch_.size(), &got), "sots_stage_launch_times_ms");
        double listed = 0.0;
        for (uint64_t i = 0; i < got; ++i) {
            hipBenchmarker_.addTimer(name, launchScratch_[i]);
            listed += launchScratch_[i];
        }
        if (got < n) hipBenchmarker_.addTimer(name, ms - listed);
    }
    bool stopRuleSet() const { return args_.targetFitness >= 0.0f || args_.stallGenerations > 0; }
    bool tracking() const { return args_.returnBestEver || args_.historyEvery > 0 || stopRuleSet(); }
    uint32_t trackFlags() const { return SOTS_TRACK_BEST_EVER | (args_.historyEvery > 0 ? (uint32_t)SOTS_TRACK_HISTORY : 0u); }
    uint32_t historyCapacity() const { return args_.historyEvery ? numGenerations / args_.historyEvery + 1 : 0; }
    void writeHistoryRows(uint32_t chunk, const std::vector<sots_gen_record> &records, uint32_t n)
    {
        if (!historyFile_) return;
        for (uint32_t i = 0; i < n; ++i) {
            const sots_gen_record &r = records[i];
            fprintf(historyFile_, "%u,%u,%.9g,%.9g,%.9g,%.9g", chunk, r.generation, r.best_fitness, r.best_ever_fitness, r.parent_mean_fitness,
                    r.parent_worst_fitness);
            for (uint32_t j = 0; j < population.numDimensions; ++j) fprintf(historyFile_, ",%.9g", r.mean_step[j]);
            fprintf(historyFile_, "\n");
        }
    }
    void harvestTimers()
    {
        if (!args_.benchmarkStages) return;
        if (group_) ctx_ = sots_group_island(group_, 0); // the instrumented island
        static const int stageOf[numKernels_] = {SOTS_STAGE_INIT, SOTS_STAGE_RECOMBINE, SOTS_STAGE_MUTATE, SOTS_STAGE_SYNTHESISE,
                                                 SOTS_STAGE_WINDOW, SOTS_STAGE_FFT, SOTS_STAGE_FITNESS, SOTS_STAGE_SORT, SOTS_STAGE_ROTATE};
        for (uint8_t k = 0; k < numKernels_; ++k) harvestStage(stageOf[k], kernelNames_[k]);
        static const std::pair<int, const char *> fused[] = {{SOTS_STAGE_FUSED_VARIATION, "recombine+mutatePopulation"},
                                                             {SOTS_STAGE_FUSED_SYNTH, "synthesise+applyWindowPopulation"},
                                                             {SOTS_STAGE_FUSED_SPECTRAL, "hipFFT+fitnessPopulation"}};
        for (const auto &f : fused) harvestStage(f.first, f.second);
        check(sots_timing_reset(ctx_), "sots_timing_reset");
    }

public:
    Evolutionary_Strategy_HIP(Evolutionary_Strategy_HIP_Arguments args)
        : Evolutionary_Strategy(args.es_args.numGenerations, args.es_args.pop.numParents, args.es_args.pop.numOffspring, args.es_args.pop.numDimensions, args.es_args.paramMin, args.es_args.paramMax, args.es_args.audioLengthLog2),
          kernelNames_({"initPopulation", "recombinePopulation", "mutatePopulation", "synthesisePopulation", "applyWindowPopulation", "hipFFT", "fitnessPopulation", "sortPopulation", "rotatePopulation"}),
          args_(args),
          hipBenchmarker_(logName(args), {"Test_Name", "Total_Time", "Average_Time", "Max_Time", "Min_Time", "Max_Difference", "Average_Difference"})
    {
        hipBenchmarker_.setVerbose(args.verbose);
        init();
    }
    ~Evolutionary_Strategy_HIP() override
    {
        if (historyFile_) fclose(historyFile_);
        if (batch_) sots_batch_destroy(batch_);
        if (group_) sots_group_destroy(group_); // owns its islands
        else if (ctx_) sots_destroy(ctx_);
        hipBenchmarker_.close();
    }
    Evolutionary_Strategy_HIP(const Evolutionary_Strategy_HIP &) = delete;
    Evolutionary_Strategy_HIP &operator=(const Evolutionary_Strategy_HIP &) = delete;

    sots_ctx *context() { return ctx_; }
    sots_group *group() { return group_; }
    uint32_t numIslands() const { return group_ ? sots_group_size(group_) : 1u; }
    uint32_t bestIsland() const { return bestIsland_; }
    Benchmarker &benchmarker() { return hipBenchmarker_; }
    const std::vector<std::vector<float>> &bestParametersPerChunk() const { return bestPerChunk_; }
    const std::vector<float> &bestFitnessPerChunk() const { return bestFitnessPerChunk_; }
    // generations after which each chunk's result was taken: numGenerations, or where its stop rule first held
    const std::vector<uint32_t> &generationsPerChunk() const { return generationsPerChunk_; }
    // samples between the chunk starts of parameterMatchAudio, and the chunks its last call matched
    uint32_t hopSize() const { return hop_; }
    uint32_t numChunks() const { return numChunks_; }
    // The whole match as audio: bestParametersPerChunk() through sots_render_overlap_add on this object's context - chunk i's
    // match stands for samples [i hop, i hop + N); where chunks overlap (hop < N) they are cross-faded with the analysis
    // window and normalised by its sum, at hop = N they follow each other as they are.  (numChunks - 1) hop + N samples.
    // With renderMode 1 or 2 the same track goes through sots_render_continuous instead: the same length, one voice from the
    // first sample to the last, chunk i's parameters reached at its centre i hop + N/2.  With 3 or 4 (the operator-graph
    // voice) through sots_render_graph_continuous, which is the same for a voice graph, and with 5 or 6 through
    // sots_render_graph_feedback, which is the same for a voice graph with feedback indices, and with 7 or 8
    // through sots_render_graph_genes, which is the same for a voice graph with voiceFeedbackGenes.
    void renderMatch(std::vector<float> &out)
    {
        const uint32_t d = population.numDimensions, chunks = (uint32_t)bestPerChunk_.size();
        out.assign((size_t)matchCoveredSamples(chunks, objective.audioLength, hop_), 0.0f);
        if (!chunks) return;
        std::vector<float> values((size_t)chunks * d);
        for (uint32_t c = 0; c < chunks; ++c) std::copy(bestPerChunk_[c].begin(), bestPerChunk_[c].begin() + d, values.begin() + (size_t)c * d);
        if (args_.renderMode >= 5u && args_.renderMode <= 8u) {
            sots_render_graph_feedback_args fa{};
            fa.struct_size = sizeof fa;
            fa.hop = hop_;
            fa.flags = args_.renderMode == 6u || args_.renderMode == 8u ? (uint32_t)SOTS_RENDER_GLIDE : 0u;
            const auto render = args_.renderMode >= 7u ? sots_render_graph_genes : sots_render_graph_feedback;
            check(render(ctx_, values.data(), values.size() * sizeof(float), chunks, &fa, out.data(), out.size()), "renderMatch");
            return;
        }
        if (args_.renderMode != 0u) {
            sots_render_continuous_args ca{};
            ca.struct_size = sizeof ca;
            ca.hop = hop_;
            ca.flags = args_.renderMode == 2u || args_.renderMode == 4u ? (uint32_t)SOTS_RENDER_GLIDE : 0u;
            const auto render = args_.renderMode >= 3u ? sots_render_graph_continuous : sots_render_continuous;
            check(render(ctx_, values.data(), values.size() * sizeof(float), chunks, &ca, out.data(), out.size()), "renderMatch");
            return;
        }
        sots_render_args ra{};
        ra.struct_size = sizeof ra;
        ra.hop = hop_;
        ra.flags = hop_ < objective.audioLength ? (uint32_t)SOTS_RENDER_WINDOWED : 0u;
        check(sots_render_overlap_add(ctx_, values.data(), values.size() * sizeof(float), chunks, &ra, out.data(), out.size()), "renderMatch");
    }
    // Frame k of `signal` (samples [k hop, k hop + N), the hop of the match) scored against the stored target of chunk k under
    // the objective, floor and weights of the match: what a listener of `signal` gets where bestFitnessPerChunk() is what the
    // search saw (a chunk's row synthesised from phase 0).  After a parameterMatchAudio through the chunk queue only: the queue
    // keeps the targets.  signal: at least (numChunks - 1) hop + N samples, e.g. renderMatch()'s.
    void scoreAgainstTargets(const std::vector<float> &signal, std::vector<float> &fitness)
    {
        if (!batch_) throw std::runtime_error("Evolutionary_Strategy_HIP: scoreAgainstTargets needs a match through the chunk queue");
        fitness.assign(numChunks_, 0.0f);
        if (sots_batch_queue_score_audio_hop(batch_, signal.data(), (uint64_t)signal.size(), hop_, fitness.data(), numChunks_) != SOTS_OK)
            throw std::runtime_error(std::string("Evolutionary_Strategy_HIP: sots_batch_queue_score_audio_hop: ") + sots_batch_last_error(batch_));
    }
    // generations really run by the last parameterMatchAudio, summed over its chunks (chunks in flight run to their batch's end)
    uint64_t generationsRun() const { return generationsRun_; }
    // bins with a positive weight (all N/2 of them without weights)
    uint32_t objectiveWeightBins() const
    {
        if (objectiveWeights_.empty()) return objective.fftHalfSize;
        return (uint32_t)std::count_if(objectiveWeights_.begin(), objectiveWeights_.end(), [](float w) { return w > 0.0f; });
    }
    // candidates evaluated per second of the last parameterMatchAudio (population x generations x chunks / wall time)
    double candidatesPerSecond() const { return candidatesPerSecond_; }

    void init() override
    {
        if (ctx_) return;
        memset(&cfg_, 0, sizeof cfg_);
        cfg_.struct_size = sizeof cfg_;
        cfg_.num_parents = population.numParents;
        cfg_.num_offspring = population.numOffspring;
        cfg_.num_dimensions = population.numDimensions;
        cfg_.audio_length_log2 = objective.audioLengthLog2;
        cfg_.num_generations = numGenerations;
        const int kind = args_.synthKind >= 0 ? args_.synthKind : kindFromDims(population.numDimensions);
        if (kind < 0) throw std::runtime_error("Evolutionary_Strategy_HIP: numDimensions must be 4, 6, 8 or 12");
        cfg_.synth_kind = (uint32_t)kind;
        const bool graphVoice = kind == SOTS_SYNTH_GRAPH;
        if (graphVoice && args_.renderMatch && (args_.renderMode == 1u || args_.renderMode == 2u))
            throw std::runtime_error("Evolutionary_Strategy_HIP: renderMode 1 and 2 (sots_render_continuous) are not available with the operator-graph voice");
        if (graphVoice && args_.deviceKernelArithmetic)
            throw std::runtime_error("Evolutionary_Strategy_HIP: deviceKernelArithmetic is not available with the operator-graph voice");
        if (!graphVoice && args_.renderMode >= 3u)
            throw std::runtime_error(args_.renderMode >= 7u
                                         ? "Evolutionary_Strategy_HIP: renderMode 7 and 8 (sots_render_graph_genes) need the operator-graph voice"
                                     : args_.renderMode >= 5u
                                         ? "Evolutionary_Strategy_HIP: renderMode 5 and 6 (sots_render_graph_feedback) need the operator-graph voice"
                                         : "Evolutionary_Strategy_HIP: renderMode 3 and 4 (sots_render_graph_continuous) need the operator-graph voice");
        if (!graphVoice && !args_.voiceWaveforms.empty())
            throw std::runtime_error("Evolutionary_Strategy_HIP: voiceWaveforms need the operator-graph voice");
        if (!graphVoice && !args_.voiceFeedback.empty())
            throw std::runtime_error("Evolutionary_Strategy_HIP: voiceFeedback needs the operator-graph voice");
        if (!graphVoice && args_.voiceFeedbackGenes)
            throw std::runtime_error("Evolutionary_Strategy_HIP: voiceFeedbackGenes need the operator-graph voice");
        if (!graphVoice && args_.graphSynthForm)
            throw std::runtime_error("Evolutionary_Strategy_HIP: graphSynthForm needs the operator-graph voice");
        if (args_.renderMode > 8u) throw std::runtime_error("Evolutionary_Strategy_HIP: renderMode must be 0 to 8");
        if (args_.voiceFeedbackGenes && args_.renderMode >= 3u && args_.renderMode <= 6u)
            throw std::runtime_error("Evolutionary_Strategy_HIP: renderMode 3 to 6 take the feedback index from the voice, not from the row: "
                                     "voiceFeedbackGenes are rendered by renderMode 0 (sots_render_overlap_add) and 7, 8 (sots_render_graph_genes)");
        cfg_.workgroup_size = args_.workgroupX * args_.workgroupY * args_.workgroupZ;
        cfg_.device = args_.deviceOrdinal;
        cfg_.gid_base = args_.gidBase;
        cfg_.seed = args_.seed;
        for (size_t i = 0; i < SOTS_MAX_DIMS; ++i) {
            cfg_.param_min[i] = i < objective.paramMins.size() ? objective.paramMins[i] : 0.0f;
            cfg_.param_max[i] = i < objective.paramMaxs.size() ? objective.paramMaxs[i] : 0.0f;
        }
        hop_ = matchHop((double)args_.hopSize, objective.audioLength); // (throws before any device work)
        objectiveWeights_ = makeObjectiveWeights(args_.objectiveWeights, objective.audioLength, (double)objective.sampleRate); // (throws before any device work)
        // (likewise: no silent fall-back to the host analysis, which would change the result's bits behind the user's back)
        const bool inFlight = args_.chunksInFlight > 1 && args_.numDevices <= 1 && population.populationLength <= 1024u;
        if (args_.deviceAnalysis && !inFlight)
            throw std::runtime_error("Evolutionary_Strategy_HIP: deviceAnalysis needs the chunks in flight (chunksInFlight > 1, one device, "
                                     "populationLength <= 1024)");
        if (!args_.matchReport.empty() && !(args_.renderMatch && inFlight && args_.chunkQueue && (args_.historyEvery == 0 || args_.historyPath.empty())))
            throw std::runtime_error("Evolutionary_Strategy_HIP: matchReport needs renderMatch and the chunk queue (chunkQueue, chunksInFlight > 1, "
                                     "one device, populationLength <= 1024, no history file)");
        if (args_.numDevices > 1) {
            std::vector<int32_t> devs = args_.devices;
            if (devs.empty())
                for (uint32_t i = 0; i < args_.numDevices; ++i) devs.push_back(args_.deviceOrdinal + (int32_t)i);
            if (devs.size() != args_.numDevices) throw std::runtime_error("Evolutionary_Strategy_HIP: devices must list numDevices entries");
            const int rc = sots_group_create(&cfg_, devs.data(), args_.numDevices, args_.numElites, args_.migrationInterval,
                                             args_.overlapMigration ? (uint32_t)SOTS_GROUP_OVERLAP : 0u, &group_);
            if (rc != SOTS_OK) throw std::runtime_error(std::string("Evolutionary_Strategy_HIP: sots_group_create: ") + sots_group_last_error(nullptr));
            ctx_ = sots_group_island(group_, 0);
        } else {
            const bool genes = graphVoice && args_.voiceFeedbackGenes != 0u;
            const int rc = genes        ? sots_create_graph_genes(&cfg_, &args_.voiceGraph, args_.voiceFeedbackGenes, &ctx_)
                           : graphVoice ? sots_create_graph(&cfg_, &args_.voiceGraph, &ctx_)
                                        : sots_create(&cfg_, &ctx_);
            if (rc != SOTS_OK)
                throw std::runtime_error(std::string("Evolutionary_Strategy_HIP: ") +
                                         (genes ? "sots_create_graph_genes: " : graphVoice ? "sots_create_graph: " : "sots_create: ") + sots_last_error(nullptr));
        }
        targetFFT_.assign(objective.fftHalfSize, 0.0f);
        if (!args_.voiceWaveforms.empty()) // (the graph voice: one device, no group)
            check(sots_set_voice_waveforms(ctx_, args_.voiceWaveforms.data(), (uint32_t)args_.voiceWaveforms.size()), "sots_set_voice_waveforms");
        if (!args_.voiceFeedback.empty())
            check(sots_set_voice_feedback(ctx_, args_.voiceFeedback.data(), (uint32_t)args_.voiceFeedback.size()), "sots_set_voice_feedback");
        if (args_.graphSynthForm != 0u) check(sots_set_graph_synth_form(ctx_, args_.graphSynthForm), "sots_set_graph_synth_form");
        if (args_.fullSortEveryGeneration)
            for (uint32_t i = 0; i < numIslands(); ++i)
                check(sots_set_sort_mode(group_ ? sots_group_island(group_, i) : ctx_, SOTS_SORT_FULL), "sots_set_sort_mode");
        if (args_.deviceKernelArithmetic)
            for (uint32_t i = 0; i < numIslands(); ++i)
                check(sots_set_synth_arithmetic(group_ ? sots_group_island(group_, i) : ctx_, SOTS_ARITH_DEVICE_KERNELS), "sots_set_synth_arithmetic");
        if (args_.survivors)
            for (uint32_t i = 0; i < numIslands(); ++i)
                check(sots_set_survivors(group_ ? sots_group_island(group_, i) : ctx_, args_.survivors), "sots_set_survivors");
        if (args_.objective != SOTS_OBJECTIVE_MAGNITUDE) {
            if (group_) {
                if (sots_group_set_objective(group_, args_.objective, args_.objectiveFloor) != SOTS_OK)
                    throw std::runtime_error(std::string("Evolutionary_Strategy_HIP: sots_group_set_objective: ") + sots_group_last_error(group_));
            } else check(sots_set_objective(ctx_, args_.objective, args_.objectiveFloor), "sots_set_objective");
        }
        if (!objectiveWeights_.empty()) {
            if (group_) {
                if (sots_group_set_objective_weights(group_, objectiveWeights_.data(), (uint32_t)objectiveWeights_.size()) != SOTS_OK)
                    throw std::runtime_error(std::string("Evolutionary_Strategy_HIP: sots_group_set_objective_weights: ") + sots_group_last_error(group_));
            } else check(sots_set_objective_weights(ctx_, objectiveWeights_.data(), (uint32_t)objectiveWeights_.size()), "sots_set_objective_weights");
        }
        check(sots_timing_enable(ctx_, args_.benchmarkStages ? 1 : 0), "sots_timing_enable");
        if (tracking()) {
            if (group_) throw std::runtime_error("Evolutionary_Strategy_HIP: returnBestEver, the history and the stop rules need numDevices = 1");
            if (args_.stopCheckInterval == 0) throw std::runtime_error("Evolutionary_Strategy_HIP: stopCheckInterval must be at least 1");
            check(sots_track(ctx_, trackFlags(), args_.historyEvery, historyCapacity()), "sots_track");
        }
        rule_.struct_size = sizeof rule_;
        rule_.check_interval = args_.stopCheckInterval;
        rule_.target_fitness = args_.targetFitness;
        rule_.stall_generations = args_.stallGenerations;
    }
    void initTargetAudio() override {}

    // "Input" arrays address the current rotation half, "Output" arrays the other one
    // (the reference transfers both buffers whole, ...OpenCL.hpp:403-430).
    void writePopulationData(void *aInputPopulationValueData, void * /*aOutputPopulationValueData*/, uint32_t aPopulationValueSize, void *aInputPopulationStepData, void * /*aOutputPopulationStepData*/, uint32_t aPopulationStepSize, void *aInputPopulationFitnessData, void * /*aOutputPopulationFitnessData*/, uint32_t aPopulationFitnessSize) override
    {
        check(sots_write_population(ctx_, (const float *)aInputPopulationValueData, aPopulationValueSize, (const float *)aInputPopulationStepData, aPopulationStepSize, (const float *)aInputPopulationFitnessData, aPopulationFitnessSize), "writePopulationData");
    }
    void readPopulationData(void *aInputPopulationValueData, void *aOutputPopulationValueData, uint32_t aPopulationValueSize, void *aInputPopulationStepData, void *aOutputPopulationStepData, uint32_t aPopulationStepSize, void *aInputPopulationFitnessData, void *aOutputPopulationFitnessData, uint32_t aPopulationFitnessSize) override
    {
        selectBestIsland();
        check(sots_read_population(ctx_, (float *)aInputPopulationValueData, aPopulationValueSize, (float *)aInputPopulationStepData, aPopulationStepSize, (float *)aInputPopulationFitnessData, aPopulationFitnessSize), "readPopulationData");
        if (aOutputPopulationValueData || aOutputPopulationStepData || aOutputPopulationFitnessData)
            check(sots_read_population_other(ctx_, (float *)aOutputPopulationValueData, aPopulationValueSize, (float *)aOutputPopulationStepData, aPopulationStepSize, (float *)aOutputPopulationFitnessData, aPopulationFitnessSize), "readPopulationData");
        // keep the host-side AoS view in step with the device (main.cpp:244 reads es->population)
        const float *v = (const float *)aInputPopulationValueData, *s = (const float *)aInputPopulationStepData, *f = (const float *)aInputPopulationFitnessData;
        if (v && s && f)
            for (uint32_t i = 0; i != population.populationLength; ++i) {
                for (uint32_t j = 0; j != population.numDimensions; ++j) {
                    *population.getValue(i, j) = v[i * population.numDimensions + j];
                    *population.getStep(i, j) = s[i * population.numDimensions + j];
                }
                *population.getFitness(i) = f[i];
            }
    }

    // aInputFFTSize: bytes of the device spectrum buffer P*(N+8)*4; the target gets aInputFFTSize/2 in the
    // reference (...OpenCL.hpp:443,452) -- here the target is always N/2 floats.
    void writeSynthesizerData(void *aOutputAudioBuffer, uint32_t aOutputAudioSize, void *aInputFFTDataBuffer, void *aInputFFTTargetBuffer, uint32_t aInputFFTSize) override
    {
        check(sots_write_synth(ctx_, (const float *)aOutputAudioBuffer, aOutputAudioSize, (const float *)aInputFFTDataBuffer, aInputFFTSize), "writeSynthesizerData");
        if (aInputFFTTargetBuffer) setTargetFFT((float *)aInputFFTTargetBuffer);
    }
    void readSynthesizerData(void *aOutputAudioBuffer, uint32_t aOutputAudioSize, void *aInputFFTDataBuffer, void *aInputFFTTargetBuffer, uint32_t aInputFFTSize) override
    {
        check(sots_read_synth(ctx_, (float *)aOutputAudioBuffer, aOutputAudioSize, (float *)aInputFFTDataBuffer, aInputFFTSize, (float *)aInputFFTTargetBuffer, aInputFFTTargetBuffer ? objective.fftHalfSize * sizeof(float) : 0), "readSynthesizerData");
    }

    void initPopulationHIP(uint32_t aChunk = 0)
    {
        if (group_) checkGroup(sots_group_init_population(group_, aChunk), "initPopulation");
        else check(sots_init_population(ctx_, aChunk), "initPopulation");
    }

    // the eight per-generation stages, each as its own launch sequence (...OpenCL.hpp:471-541); a group of
    // islands runs the fused loop (its exchange sits between generations)
    void executeGeneration() override
    {
        if (group_) checkGroup(sots_group_execute_generations(group_, 1), "executeGeneration");
        else check(sots_execute_generation(ctx_), "executeGeneration");
    }
    void executeAllGenerations() override
    {
        lastRun_ = numGenerations;
        if (stopRuleSet()) { // (the fused loop, in blocks of stopCheckInterval generations)
            check(sots_execute_until(ctx_, numGenerations, &rule_, &lastRun_), "executeAllGenerations");
        } else if (group_) {
            checkGroup(sots_group_execute_generations(group_, numGenerations), "executeAllGenerations");
        } else if (args_.fusedGenerations) {
            check(sots_execute_generations(ctx_, numGenerations), "executeAllGenerations");
        } else {
            for (uint32_t i = 0; i != numGenerations; ++i) executeGeneration();
        }
    }

    void setTargetAudio(float *aTargetAudio, uint32_t aTargetAudioLength)
    {
        // host: double window -> fp64 DFT -> magnitudes (Objective::calculateFFT), then H2D (...OpenCL.hpp:563-570)
        targetAudioLength = aTargetAudioLength;
        objective.calculateFFT(aTargetAudio, targetFFT_.data());
        if (group_) checkGroup(sots_group_set_target_spectrum(group_, targetFFT_.data(), objective.fftHalfSize), "setTargetAudio");
        else check(sots_set_target_spectrum(ctx_, targetFFT_.data(), objective.fftHalfSize), "setTargetAudio");
    }
    void setTargetFFT(float *aTargetFFT) override
    {
        std::copy(aTargetFFT, aTargetFFT + objective.fftHalfSize, targetFFT_.begin());
        if (group_) checkGroup(sots_group_set_target_spectrum(group_, targetFFT_.data(), objective.fftHalfSize), "setTargetFFT");
        else check(sots_set_target_spectrum(ctx_, targetFFT_.data(), objective.fftHalfSize), "setTargetFFT");
    }

    void parameterMatchAudio(float *aTargetAudio, uint32_t aTargetAudioLength) override
    {
        // every N-sample chunk is matched from a fresh population (...OpenCL.hpp:572-610); the chunks start hop_ samples apart
        // (the reference's N unless type.HIP.hopSize says otherwise)
        chunkSize_ = objective.audioLength;
        numChunks_ = matchChunkCount(aTargetAudioLength, chunkSize_, hop_); // (hop = N: aTargetAudioLength / N)
        bestPerChunk_.clear();
        bestFitnessPerChunk_.clear();
        generationsPerChunk_.clear();
        generationsRun_ = 0;
        if (historyFile_) fclose(historyFile_), historyFile_ = nullptr;
        if (args_.historyEvery > 0 && !args_.historyPath.empty()) {
            historyFile_ = fopen(args_.historyPath.c_str(), "w");
            if (!historyFile_) throw std::runtime_error("Evolutionary_Strategy_HIP: cannot write " + args_.historyPath);
            fprintf(historyFile_, "chunk,generation,best,best_ever,parent_mean,parent_worst");
            for (uint32_t j = 0; j < population.numDimensions; ++j) fprintf(historyFile_, ",step_%u", j);
            fprintf(historyFile_, "\n");
        }
        std::vector<sots_gen_record> records(historyCapacity());

        const bool batched = args_.chunksInFlight > 1 && !group_ && population.populationLength <= 1024u;
        if (args_.chunksInFlight > 1 && !batched && args_.verbose)
            printf("chunksInFlight %u: %s, matching chunk by chunk\n", args_.chunksInFlight,
                   group_ ? "numDevices > 1" : "populationLength > 1024");
        hipBenchmarker_.startTimer("Total Audio Analysis Time");
        const bool queued = batched && args_.chunkQueue && !historyFile_ && numGenerations > 0 && numChunks_ > 0;
        if (batched && args_.chunkQueue && historyFile_ && args_.verbose)
            printf("chunkQueue: a history file is written, matching batch by batch\n");
        if (args_.carryRows && !queued)
            throw std::runtime_error("Evolutionary_Strategy_HIP: carryRows needs the chunk queue (chunkQueue, chunksInFlight > 1, one device, "
                                     "populationLength <= 1024, no history file)");
        if (queued) {
            matchChunkQueue(aTargetAudio);
        } else if (batched) {
            matchChunksInFlight(aTargetAudio);
        } else {
            for (uint32_t i = 0; i < numChunks_; i++) {
                setTargetAudio(&aTargetAudio[(size_t)hop_ * i], chunkSize_);
                initPopulationHIP(i);
                executeAllGenerations();
                if (group_) checkGroup(sots_group_synchronize(group_), "synchronize");
                else check(sots_synchronize(ctx_), "synchronize");
                if (args_.verbose) printf("Audio chunk %u evaluated:\n", i);
                printBest();
                generationsPerChunk_.push_back(lastRun_);
                generationsRun_ += lastRun_;
                if (stopRuleSet() && args_.verbose) printf("Generations run: %u\n", lastRun_);
                if (historyFile_) {
                    uint32_t got = 0;
                    check(sots_read_history(ctx_, records.data(), (uint32_t)records.size(), &got, nullptr), "sots_read_history");
                    writeHistoryRows(i, records, got);
                }
                harvestTimers();
            }
        }
        hipBenchmarker_.pauseTimer("Total Audio Analysis Time");
        const double totalMs = hipBenchmarker_.totalMs("Total Audio Analysis Time");
        if (historyFile_) fclose(historyFile_), historyFile_ = nullptr;
        // (generationsRun_ = numGenerations x numChunks_ unless a stop rule ended chunks early)
        candidatesPerSecond_ = totalMs > 0.0 ? (double)population.populationLength * numIslands() * (double)generationsRun_ / (totalMs * 1e-3) : 0.0;
        if (args_.verbose) printf("Candidates evaluated per second: %.6g\n", candidatesPerSecond_);

        for (uint8_t k = 1; k < numKernels_; ++k)
            if (hipBenchmarker_.count(kernelNames_[k])) hipBenchmarker_.elapsedTimer(kernelNames_[k]);
        for (const char *name : {"recombine+mutatePopulation", "synthesise+applyWindowPopulation", "hipFFT+fitnessPopulation"})
            if (hipBenchmarker_.count(name)) hipBenchmarker_.elapsedTimer(name);
        hipBenchmarker_.elapsedTimer("Total Audio Analysis Time");
    }

    // rotation-aware (the reference reads offset 0 whatever the rotation index, ...OpenCL.hpp:612-631)
    void printBest() override
    {
        selectBestIsland();
        const uint32_t d = population.numDimensions;
        if (args_.returnBestEver) { // the best individual any generation produced, not row 0 of the last one
            std::vector<float> best(d);
            float fitness = 0.0f;
            check(sots_read_best_ever(ctx_, best.data(), best.size() * sizeof(float), nullptr, 0, &fitness, nullptr), "printBest");
            recordBest(best.data(), fitness);
            return;
        }
        std::vector<float> v((size_t)population.populationLength * d), f(population.populationLength);
        check(sots_read_population(ctx_, v.data(), v.size() * sizeof(float), nullptr, 0, f.data(), f.size() * sizeof(float)), "printBest");
        recordBest(v.data(), f[0]);
    }

private:
    // one chunk's result: kept for bestParametersPerChunk() and printed (printBest's lines)
    void recordBest(const float *bestValues, float bestFitness)
    {
        const uint32_t d = population.numDimensions;
        std::vector<float> best(bestValues, bestValues + d);
        bestPerChunk_.push_back(best);
        bestFitnessPerChunk_.push_back(bestFitness);
        if (!args_.verbose) return;
        const std::vector<float> scaled = objective.scaleParams(best);
        printf("Best parameters found:\n");
        for (uint32_t j = 0; j < d && j < scaled.size(); ++j) printf(" p%u = %f\n", j, scaled[j]);
        printf("Best fitness: %g\n\n", bestFitness);
    }

    // parameterMatchAudio through the chunk queue: every chunk's target (Objective::calculateFFT, as setTargetAudio) goes to the
    // device, ONE sots_batch_queue_run matches them all in chunksInFlight slots, and the results come back together.  The
    // last chunk's population, as it was when that chunk stopped, is kept and written into the context, so that
    // readPopulationData and printBest read what they read after the chunk-by-chunk loop.
    void matchChunkQueue(const float *aTargetAudio)
    {
        const uint32_t half = objective.fftHalfSize, d = population.numDimensions, P = population.populationLength;
        if (!batch_) createBatch();
        auto checkBatch = [&](int rc, const char *what) {
            if (rc != SOTS_OK) throw std::runtime_error(std::string("Evolutionary_Strategy_HIP: ") + what + ": " + sots_batch_last_error(batch_));
        };
        if (args_.deviceKernelArithmetic) checkBatch(sots_batch_set_synth_arithmetic(batch_, SOTS_ARITH_DEVICE_KERNELS), "sots_batch_set_synth_arithmetic");
        checkBatch(sots_batch_set_survivors(batch_, args_.survivors), "sots_batch_set_survivors");
        checkBatch(sots_batch_set_objective(batch_, args_.objective, args_.objectiveFloor), "sots_batch_set_objective");
        if (!objectiveWeights_.empty())
            checkBatch(sots_batch_set_objective_weights(batch_, objectiveWeights_.data(), (uint32_t)objectiveWeights_.size()), "sots_batch_set_objective_weights");
        checkBatch(sots_batch_track(batch_, SOTS_TRACK_BEST_EVER, 0, 0), "sots_batch_track"); // (the queue keeps the best-ever record itself)
        const uint32_t segment = !args_.carryRows ? 0u : args_.segmentChunks ? args_.segmentChunks : (numChunks_ + args_.chunksInFlight - 1u) / args_.chunksInFlight;
        checkBatch(sots_batch_queue_set_carry(batch_, args_.carryRows, segment), "sots_batch_queue_set_carry");
        if (args_.carryRows && args_.verbose) printf("Carried rows: %u, in segments of %u chunks\n", args_.carryRows, segment);
        if (args_.deviceAnalysis) { // the samples the chunks cover go up once; the device makes the spectra where the queue stores them
            checkBatch(sots_batch_set_analysis(batch_, SOTS_ANALYSIS_DEVICE), "sots_batch_set_analysis");
            checkBatch(sots_batch_queue_targets_audio_hop(batch_, aTargetAudio, matchCoveredSamples(numChunks_, objective.audioLength, hop_), hop_, numChunks_),
                       "sots_batch_queue_targets_audio_hop");
        } else {
            std::vector<float> mags((size_t)numChunks_ * half);
            for (uint32_t c = 0; c < numChunks_; ++c) objective.calculateFFT((float *)&aTargetAudio[(size_t)hop_ * c], mags.data() + (size_t)c * half);
            checkBatch(sots_batch_queue_targets_spectra(batch_, mags.data(), (uint64_t)mags.size(), numChunks_), "sots_batch_queue_targets_spectra");
        }
        sots_queue_stats stats{};
        stats.struct_size = sizeof stats;
        checkBatch(sots_batch_queue_run(batch_, 0, numGenerations, stopRuleSet() ? &rule_ : nullptr, numChunks_ - 1, &stats), "sots_batch_queue_run");
        std::vector<sots_chunk_result> results(numChunks_);
        uint32_t got = 0;
        checkBatch(sots_batch_queue_results(batch_, results.data(), numChunks_, &got), "sots_batch_queue_results");
        if (got != numChunks_) throw std::runtime_error("Evolutionary_Strategy_HIP: sots_batch_queue_results: results missing");
        generationsRun_ = stats.chunk_generations;
        for (uint32_t c = 0; c < numChunks_; ++c) {
            const sots_chunk_result &r = results[c];
            if (args_.verbose) printf("Audio chunk %u evaluated:\n", c);
            if (args_.returnBestEver) recordBest(r.best_ever_values, r.best_ever_fitness);
            else recordBest(r.last_values, r.last_fitness);
            generationsPerChunk_.push_back(r.generations_run);
            if (stopRuleSet() && args_.verbose) printf("Generations run: %u\n", r.generations_run);
        }
        std::vector<float> v((size_t)P * d), s((size_t)P * d), f(P);
        checkBatch(sots_batch_queue_read_kept_population(batch_, v.data(), v.size() * sizeof(float), s.data(), s.size() * sizeof(float), f.data(),
                                                         f.size() * sizeof(float)), "sots_batch_queue_read_kept_population");
        check(sots_write_population(ctx_, v.data(), v.size() * sizeof(float), s.data(), s.size() * sizeof(float), f.data(), f.size() * sizeof(float)),
              "writePopulationData");
    }

    // parameterMatchAudio with chunksInFlight chunks per batch (the last batch may be ragged): per batch the targets
    // (Objective::calculateFFT, as setTargetAudio), one initialisation, the generations, ONE synchronisation and the best
    // rows.  Afterwards the context holds the last chunk's population, as after the chunk-by-chunk loop, so that
    // readPopulationData and printBest read what they read there (the current rotation half).
    void matchChunksInFlight(const float *aTargetAudio)
    {
        const uint32_t half = objective.fftHalfSize, d = population.numDimensions, P = population.populationLength;
        const uint32_t perBatch = std::min(args_.chunksInFlight, numChunks_);
        if (perBatch == 0) return;
        if (!batch_) createBatch();
        auto checkBatch = [&](int rc, const char *what) {
            if (rc != SOTS_OK) throw std::runtime_error(std::string("Evolutionary_Strategy_HIP: ") + what + ": " + sots_batch_last_error(batch_));
        };
        if (args_.deviceKernelArithmetic) checkBatch(sots_batch_set_synth_arithmetic(batch_, SOTS_ARITH_DEVICE_KERNELS), "sots_batch_set_synth_arithmetic");
        checkBatch(sots_batch_set_survivors(batch_, args_.survivors), "sots_batch_set_survivors");
        checkBatch(sots_batch_set_objective(batch_, args_.objective, args_.objectiveFloor), "sots_batch_set_objective");
        if (!objectiveWeights_.empty())
            checkBatch(sots_batch_set_objective_weights(batch_, objectiveWeights_.data(), (uint32_t)objectiveWeights_.size()), "sots_batch_set_objective_weights");
        if (tracking()) checkBatch(sots_batch_track(batch_, trackFlags(), args_.historyEvery, historyCapacity()), "sots_batch_track");
        if (args_.deviceAnalysis) checkBatch(sots_batch_set_analysis(batch_, SOTS_ANALYSIS_DEVICE), "sots_batch_set_analysis");
        std::vector<float> mags((size_t)perBatch * half), values((size_t)perBatch * d), fitness(perBatch);
        std::vector<float> nowValues((size_t)perBatch * d), nowFitness(perBatch), everFitness(perBatch);
        std::vector<uint32_t> nowGeneration(perBatch), stoppedAt(perBatch);
        std::vector<sots_gen_record> records(historyCapacity());
        // every active chunk's result as of now: the best-ever record, or row 0 of the current generation
        auto readResults = [&](uint32_t n, float *v, float *f) {
            if (args_.returnBestEver)
                checkBatch(sots_batch_read_best_ever(batch_, v, (size_t)n * d * sizeof(float), nullptr, 0, f, (size_t)n * sizeof(float), nullptr, 0),
                           "sots_batch_read_best_ever");
            else
                checkBatch(sots_batch_read_best(batch_, v, (size_t)n * d * sizeof(float), f, (size_t)n * sizeof(float)), "sots_batch_read_best");
        };
        uint32_t last = 0;
        for (uint32_t first = 0; first < numChunks_; first += perBatch) {
            const uint32_t n = std::min(perBatch, numChunks_ - first);
            if (args_.deviceAnalysis) { // the batch's samples, from its first chunk's start on, in one upload
                checkBatch(sots_batch_set_target_audio_hop(batch_, aTargetAudio + (size_t)hop_ * first,
                                                           (uint32_t)matchCoveredSamples(n, objective.audioLength, hop_), hop_, n),
                           "sots_batch_set_target_audio_hop");
            } else {
                for (uint32_t c = 0; c < n; ++c) objective.calculateFFT((float *)&aTargetAudio[(size_t)hop_ * (first + c)], mags.data() + (size_t)c * half);
                checkBatch(sots_batch_set_target_spectra(batch_, mags.data(), n * half, n), "sots_batch_set_target_spectra");
            }
            checkBatch(sots_batch_init_population(batch_, first), "sots_batch_init_population");
            uint32_t done = 0;
            if (stopRuleSet()) {
                // one block of stopCheckInterval generations per call; a chunk whose rule holds at a boundary has its result
                // taken there - what the chunk-by-chunk loop reports for it - and the batch goes on until every chunk has
                std::fill(stoppedAt.begin(), stoppedAt.begin() + n, 0u);
                uint32_t open = n;
                while (done < numGenerations && open) {
                    uint32_t run = 0;
                    checkBatch(sots_batch_execute_until(batch_, std::min(args_.stopCheckInterval, numGenerations - done), &rule_, &run),
                               "sots_batch_execute_until");
                    done += run;
                    checkBatch(sots_batch_read_best_ever(batch_, nullptr, 0, nullptr, 0, everFitness.data(), (size_t)n * sizeof(float),
                                                         nowGeneration.data(), (size_t)n * sizeof(uint32_t)), "sots_batch_read_best_ever");
                    bool fetched = false;
                    for (uint32_t c = 0; c < n; ++c) {
                        if (stoppedAt[c]) continue;
                        if (sots_stop_rule_holds(&rule_, everFitness[c], nowGeneration[c], done) != 1 && done < numGenerations) continue;
                        if (!fetched) readResults(n, nowValues.data(), nowFitness.data()), fetched = true;
                        std::copy(nowValues.begin() + (size_t)c * d, nowValues.begin() + (size_t)(c + 1) * d, values.begin() + (size_t)c * d);
                        fitness[c] = nowFitness[c];
                        stoppedAt[c] = done;
                        --open;
                    }
                }
            } else {
                checkBatch(sots_batch_execute_generations(batch_, numGenerations), "sots_batch_execute_generations");
                checkBatch(sots_batch_synchronize(batch_), "sots_batch_synchronize");
                readResults(n, values.data(), fitness.data());
                done = numGenerations;
                std::fill(stoppedAt.begin(), stoppedAt.begin() + n, done);
            }
            generationsRun_ += (uint64_t)done * n;
            for (uint32_t c = 0; c < n; ++c) {
                if (args_.verbose) printf("Audio chunk %u evaluated:\n", first + c);
                recordBest(values.data() + (size_t)c * d, fitness[c]);
                generationsPerChunk_.push_back(stoppedAt[c]);
                if (stopRuleSet() && args_.verbose) printf("Generations run: %u\n", stoppedAt[c]);
                if (historyFile_) {
                    uint32_t got = 0;
                    checkBatch(sots_batch_read_history(batch_, c, records.data(), (uint32_t)records.size(), &got, nullptr), "sots_batch_read_history");
                    writeHistoryRows(first + c, records, got);
                }
            }
            last = n - 1;
        }
        std::vector<float> v((size_t)P * d), s((size_t)P * d), f(P);
        checkBatch(sots_batch_read_population(batch_, last, v.data(), v.size() * sizeof(float), s.data(), s.size() * sizeof(float), f.data(),
                                              f.size() * sizeof(float)), "sots_batch_read_population");
        check(sots_write_population(ctx_, v.data(), v.size() * sizeof(float), s.data(), s.size() * sizeof(float), f.data(), f.size() * sizeof(float)),
              "writePopulationData");
    }
};

#endif
