// sots_match.cpp -- command-line driver with the reference's interface (main.cpp:25-305):
//     sots_match -j parameters.json
// Reads the reference's parameters.json schema (general / audio / evolutionary / type), with
// "type": {"implementation": "HIP", "HIP": {"workgroupSize", "device", "seed", "synth", "voiceGraph", "voiceWaveforms", "voiceFeedback", "numDevices", "numElites",
// "migrationInterval", "overlapMigration", "devices", "fullSortEveryGeneration", "deviceKernelArithmetic", "chunksInFlight", "chunkQueue",
// "carryRows", "segmentChunks", "survivors", "objective", "objectiveFloor", "objectiveWeights", "hopSize", "renderMatch", "renderMode", "matchPath", "deviceAnalysis", "matchReport", "returnBestEver", "historyEvery", "historyPath", "targetFitness", "stallGenerations", "stopCheckInterval"}},
// builds the target from "params" (synthesised) or "audio" (a mono WAV file), matches every
// N-sample chunk with Evolutionary_Strategy_HIP, writes inputGenerated.wav and the
// outputAudioPath rendering of the best match, and prints the best parameters.
//   "hopSize"     samples between chunk starts: chunk i is samples [i hopSize, i hopSize + N).  0 or absent: N, the
//                 reference's chunking; otherwise a whole number in N / 64 (rounded up) .. N, which need not divide N.
//                 A file of L samples has (L - N) / hopSize + 1 chunks.
//   "renderMatch" true: outputAudioPath receives the rendering of the WHOLE match, (chunks - 1) hopSize + N samples - every
//                 chunk's best parameters synthesised and overlap-added on the GPU (sots_render_overlap_add: cross-faded
//                 with the analysis window where chunks overlap, end to end at hopSize = N) - instead of 2^14 samples of
//                 the last chunk's.
//   "renderMode"  which renderer "renderMatch" uses: "overlapAdd" (the default, as above), "continuous" - the parameter track
//                 as ONE voice whose oscillators never restart (sots_render_continuous): no phase jumps between chunks and
//                 no comb filter where they overlap; chunk i's parameters hold around its centre i hopSize + N/2 - or
//                 "continuousGlide", the same with the parameters interpolated from centre to centre.  Same length.
//                 Ignored without "renderMatch"; not available with "deviceKernelArithmetic".  With "synth": "graph" the two
//                 are "graphContinuous" and "graphContinuousGlide" (sots_render_graph_continuous): the same rendering for
//                 any voice graph and its waveforms, not with a "voiceFeedback" other than 0; refused with any other synth.
//                 "graphFeedback" and "graphFeedbackGlide" (sots_render_graph_feedback) are those two with any "voiceFeedback".
//                 "graphGenes" and "graphGenesGlide" (sots_render_graph_genes) are those two with "voiceFeedbackGenes" too: every
//                 chunk's match with its own feedback indices, held or interpolated like its other parameters.
//   "voiceGraph"  with "synth": "graph", the operator-graph voice (sots_create_graph): {"operators": n, "modulators":
//                 [[...], ...], "carriers": [...]} - modulators[j] lists the operators that modulate operator j (each
//                 below j), carriers the operators that are heard; gene 2j is operator j's frequency, gene 2j+1 its level,
//                 so evolutionary.numDimensions is 2 n and paramMins / paramMaxs hold 2 n entries.  One device; not with
//                 "continuous" / "continuousGlide" rendering (its own: "graphContinuous" / "graphContinuousGlide") or
//                 "deviceKernelArithmetic".
//   "voiceWaveforms" with "voiceGraph": one waveform per operator, each of "sine" (the default), "half", "abs", "pulse",
//                 "even", "absEven", "square", "saw" - shapes cut out of the one sine table (sots_set_voice_waveforms), so
//                 that an operator emits a harmonic series.  Search, rendering, report and the host's own synthesiser use it.
//   "voiceFeedbackGenes" with "voiceGraph": one 0 or 1 per operator; 1 makes that operator's feedback index a gene of the
//                 individual (sots_create_graph_genes): "numDimensions" is 2 n + the number of 1s, "paramMins" / "paramMaxs"
//                 carry the genes' ranges, within [0, 2], behind the others, and "matchPath" writes the index per chunk with
//                 the other columns.  Not on an operator with a "voiceFeedback" other than 0; of the "graph..." renderModes only
//                 "graphGenes" and "graphGenesGlide" (sots_render_graph_genes) render such a match.
//   "voiceFeedback" with "voiceGraph": one feedback index in [0, 2] per operator, 0 (the default) for none: the operator's phase
//                 is offset by index x W / 2 pi x the mean of its own last two values (sots_set_voice_feedback), so that a
//                 sine operator emits a harmonic series whose brightness follows the index.  Used wherever the waveforms are.
//   "graphSynthForm" with "voiceGraph": "auto" (the default), "lanes" or "timeParallel": which synthesis kernel the graph
//                 voice runs (sots_set_graph_synth_form) - the same audio bit for bit; refused with any other synth.
//   "matchPath"   a CSV of the parameter track, one row per chunk:
//                 chunk,start_sample,generations,fitness,u0..u{D-1},p0..p{D-1} - u the unit-range genes (%.9g: the fp32
//                 bits), p the scaled parameters; with returnBestEver the best-ever individual of each chunk.
//   "deviceAnalysis" true: the chunks' target spectra come from one upload of the audio and an fp32 transform on the GPU
//                 instead of the host's fp64 one, chunk by chunk.  Not the same bits, so not the same match: off by default.
//                 Needs "chunksInFlight" > 1 (one device, a population of at most 1024).
//   "matchReport" a CSV chunk,fitness,rendered_fitness (%.9g), one row per chunk: the fitness the search reported for the
//                 chunk, and that of the RENDERED signal's frame at the chunk's place against the same target.  Needs
//                 "renderMatch" and "chunkQueue".
//
// The JSON reader and the WAV reader/writer are small built-ins: the reference's
// dependencies (nlohmann json, libsndfile, AudioFile) are not vendored and not needed.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "Evolutionary_Strategy_HIP.hpp"
#include "Match_JSON.hpp"
#include "Wav_IO.hpp"

static void show_usage(const std::string &name)
{
    std::cerr << "Usage: " << name << " -j <parameters.json>\n"
              << "  -h, --help        this text\n"
              << "  -j, --json PATH   configuration in the reference's parameters.json schema;\n"
              << "                    type.implementation must be \"HIP\" (or any value with --force-hip)\n"
              << "  --force-hip       run the HIP backend whatever type.implementation says\n";
}

int main(int argc, char *argv[])
{
    try {
        std::string jsonPath;
        bool forceHip = false;
        for (int i = 1; i < argc; ++i) {
            const std::string arg = argv[i];
            if (arg == "-h" || arg == "--help") { show_usage(argv[0]); return 0; }
            else if ((arg == "-j" || arg == "--json") && i + 1 < argc) jsonPath = argv[++i];
            else if (arg == "--force-hip") forceHip = true;
        }
        if (jsonPath.empty()) { show_usage(argv[0]); return 1; }
        std::ifstream ifs(jsonPath);
        if (!ifs) throw std::runtime_error("cannot open " + jsonPath);
        std::stringstream buf;
        buf << ifs.rdbuf();
        const std::string text = buf.str();
        const Json j = JsonParser(text).value();

        const std::string implementation = j["type"]["implementation"].str;
        if (implementation != "HIP" && !forceHip)
            throw std::runtime_error("type.implementation is \"" + implementation + "\": this build carries the HIP backend only (use --force-hip)");
        const std::string outputAudioPath = j["general"]["outputAudioPath"].str;
        const bool verbose = !j["general"].has("isDebug") || j["general"]["isDebug"].b;
        const uint32_t audioLengthLog2 = (uint32_t)j["audio"]["audioLengthLog2"].number();
        const Json &evo = j["evolutionary"];

        Evolutionary_Strategy_HIP_Arguments args;
        args.es_args.pop.numParents = (uint32_t)evo["numParents"].number();
        args.es_args.pop.numOffspring = (uint32_t)evo["numOffspring"].number();
        args.es_args.pop.numDimensions = (uint32_t)evo["numDimensions"].number();
        args.es_args.pop.populationLength = args.es_args.pop.numParents + args.es_args.pop.numOffspring;
        args.es_args.pop.populationSize = args.es_args.pop.populationLength * sizeof(float);
        args.es_args.numGenerations = (uint32_t)evo["numGenerations"].number();
        args.es_args.paramMin = evo["paramMins"].floats();
        args.es_args.paramMax = evo["paramMaxs"].floats();
        args.es_args.audioLengthLog2 = audioLengthLog2;
        args.verbose = verbose;
        // general.isBenchmarking (parameters.json:7, main.cpp:85): per-stage hipEvent timing on / off
        if (j["general"].has("isBenchmarking")) args.benchmarkStages = j["general"]["isBenchmarking"].b;
        if (j["type"].has("HIP")) {
            const Json &h = j["type"]["HIP"];
            if (h.has("workgroupSize")) args.workgroupX = (uint32_t)h["workgroupSize"].number();
            if (h.has("device")) args.deviceOrdinal = (int32_t)h["device"].number();
            if (h.has("seed")) args.seed = (uint64_t)h["seed"].number();
            // island model: one island of numParents + numOffspring per device, elites all-gathered over RCCL
            if (h.has("numDevices")) args.numDevices = (uint32_t)h["numDevices"].number();
            if (h.has("numElites")) args.numElites = (uint32_t)h["numElites"].number();
            if (h.has("migrationInterval")) args.migrationInterval = (uint32_t)h["migrationInterval"].number();
            if (h.has("overlapMigration")) args.overlapMigration = h["overlapMigration"].b;
            if (h.has("fullSortEveryGeneration")) args.fullSortEveryGeneration = h["fullSortEveryGeneration"].b;
            if (h.has("deviceKernelArithmetic")) args.deviceKernelArithmetic = h["deviceKernelArithmetic"].b;
            // chunks matched at once (one population per chunk, the launches of one; Evolutionary_Strategy_HIP_Arguments)
            if (h.has("chunksInFlight")) args.chunksInFlight = (uint32_t)h["chunksInFlight"].number();
            // ... through one queue: a slot takes the next chunk as soon as its chunk's stop rule holds
            if (h.has("chunkQueue")) args.chunkQueue = h["chunkQueue"].b;
            // ... whose chunks, in segments of segmentChunks, start from their predecessor's best rows (Match_JSON.hpp)
            (void)readCarryKeys(h, args.es_args.pop.numParents, args.carryRows, args.segmentChunks);
            // elitist survival: the best `survivors` rows are carried unchanged into each generation (0: the reference's strategy)
            if (h.has("survivors")) {
                // a value above every population goes to the library as the largest count, which refuses it with its own text
                const double k = h["survivors"].number();
                if (!(k >= 0.0)) throw std::runtime_error("parameters.json: type.HIP.survivors must not be negative");
                args.survivors = k >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)k;
            }
            // the spectral objective: "magnitude" (the reference's, the default) or "logMagnitude" with its floor (Match_JSON.hpp)
            args.objectiveGiven = readObjectiveKeys(h, args.objective, args.objectiveFloor);
            // per-bin weights of that objective: {"bandHz": [lo, hi]}, "aWeighting" or an array of N/2 numbers (Match_JSON.hpp)
            (void)readObjectiveWeightsKey(h, args.objectiveWeights);
            // analysis at a hop, the rendering of the whole match and the parameter track (Match_track.hpp; header comment)
            (void)readHopSizeKey(h, 1u << audioLengthLog2, args.hopSize);
            if (h.has("renderMatch")) args.renderMatch = h["renderMatch"].b;
            (void)readRenderModeKey(h, args.renderMode);
            if (args.renderMatch && (args.renderMode == 1u || args.renderMode == 2u) && h.has("deviceKernelArithmetic") && h["deviceKernelArithmetic"].b)
                throw std::runtime_error("parameters.json: type.HIP.renderMode \"continuous\" and \"continuousGlide\" are not available with deviceKernelArithmetic");
            if (h.has("matchPath")) args.matchPath = h["matchPath"].str;
            // the targets analysed on the device, and the report that scores the rendered match against them (Match_JSON.hpp)
            (void)readAnalysisKeys(h, (uint64_t)args.es_args.pop.numParents + args.es_args.pop.numOffspring, args.deviceAnalysis, args.matchReport);
            // run record (Evolutionary_Strategy_HIP_Arguments): the best individual any generation produced, a history CSV,
            // and stopping a chunk early on a fitness target or a stall
            if (h.has("returnBestEver")) args.returnBestEver = h["returnBestEver"].b;
            if (h.has("historyEvery")) args.historyEvery = (uint32_t)h["historyEvery"].number();
            if (h.has("historyPath")) args.historyPath = h["historyPath"].str;
            if (h.has("targetFitness")) args.targetFitness = (float)h["targetFitness"].number();
            if (h.has("stallGenerations")) args.stallGenerations = (uint32_t)h["stallGenerations"].number();
            if (h.has("stopCheckInterval")) args.stopCheckInterval = (uint32_t)h["stopCheckInterval"].number();
            if (h.has("devices"))
                for (const Json &dv : h["devices"].arr) args.devices.push_back((int32_t)dv.number());
            if (h.has("synth")) {
                const std::string s = h["synth"].str;
                args.synthKind = s == "2op" ? SOTS_SYNTH_2OP : s == "3op_series" ? SOTS_SYNTH_3OP_SERIES
                               : s == "triple_parallel" ? SOTS_SYNTH_TRIPLE_PAR : s == "4op_series" ? SOTS_SYNTH_4OP_SERIES
                               : s == "graph" ? SOTS_SYNTH_GRAPH : -1;
            }
            // the operator-graph voice: "synth": "graph" with "voiceGraph" (Match_JSON.hpp)
            const bool graphVoice = readVoiceGraphKeys(h, args.es_args.pop.numDimensions, args.renderMatch, args.renderMode, args.voiceGraph);
            // ... and its operators' waveforms: "voiceWaveforms", one name per operator (Match_JSON.hpp)
            (void)readVoiceWaveformsKey(h, graphVoice, args.voiceGraph.num_operators, args.voiceWaveforms);
            // ... and their feedback indices: "voiceFeedback", one number per operator (Match_JSON.hpp)
            (void)readVoiceFeedbackKey(h, graphVoice, args.voiceGraph.num_operators, args.voiceFeedback);
            // ... or chosen operators' indices as genes of the individual: "voiceFeedbackGenes", a 0 or 1 per operator (Match_JSON.hpp)
            (void)readVoiceFeedbackGenesKey(h, graphVoice, args.voiceGraph.num_operators, args.voiceFeedback, args.es_args.pop.numDimensions,
                                            args.es_args.paramMin.size(), args.es_args.paramMax.size(), args.renderMode, args.voiceFeedbackGenes);
            // ... and which synthesis kernel it runs: "graphSynthForm", "auto", "lanes" or "timeParallel" (Match_JSON.hpp)
            (void)readGraphSynthFormKey(h, graphVoice, args.graphSynthForm);
            // "graphContinuous" / "graphContinuousGlide" rendering: the graph voice's, without feedback (Match_JSON.hpp)
            checkGraphRenderMode(args.renderMode, graphVoice, args.renderMatch, args.voiceFeedback);
        }
        const uint32_t D = args.es_args.pop.numDimensions;
        Evolutionary_Strategy_HIP *hipEs = new Evolutionary_Strategy_HIP(args);
        std::unique_ptr<Evolutionary_Strategy> es(hipEs);
        const sots_voice_graph &vg = args.voiceGraph;
        auto synthesise = [&](Objective &obj, const std::vector<float> &p, float *out) {
            if (args.synthKind == SOTS_SYNTH_GRAPH)
                obj.synthesiseAudioGraph(vg.num_operators, vg.carriers, vg.modulators, args.voiceWaveforms.empty() ? nullptr : args.voiceWaveforms.data(),
                                         args.voiceFeedback.empty() ? nullptr : args.voiceFeedback.data(), args.voiceFeedbackGenes, p, out);
            else if (D == 4) obj.synthesiseAudio(p, out);
            else if (D == 6) obj.synthesiseAudioDoubleSeries(p, out);
            else if (D == 8) obj.synthesiseAudioQuadSeries(p, out);
            else obj.synthesiseAudioTriple(p, out);
        };

        // target (main.cpp:198-228): a WAV file, or audio generated from known parameters
        const uint32_t N = 1u << audioLengthLog2;
        std::vector<float> targetAudio;
        if (j["type"]["input"].str == "audio") {
            targetAudio = readAudioFile(j["type"]["audio"].str);
            if (targetAudio.size() < N) targetAudio.resize(N, 0.0f);
        } else {
            const std::vector<float> raw = j["type"]["params"].floats();
            if (raw.size() < D) throw std::runtime_error("type.params needs numDimensions entries");
            std::vector<float> unit(D);
            for (uint32_t i = 0; i < D; ++i) {
                const uint32_t s = D == 12 && args.synthKind != SOTS_SYNTH_GRAPH ? (i & 3u) : i;
                const float lo = args.es_args.paramMin[s], hi = args.es_args.paramMax[s];
                unit[i] = (raw[i] - lo) / (hi - lo);
            }
            targetAudio.resize(N);
            synthesise(es->objective, unit, targetAudio.data());
            outputAudioFile("inputGenerated.wav", targetAudio.data(), N);
        }

        if (args.objectiveGiven) // (without the keys: not a byte more than before)
            printf("Objective: %s, floor %g\n", args.objective == SOTS_OBJECTIVE_LOG_MAGNITUDE ? "logMagnitude" : "magnitude", (double)args.objectiveFloor);
        if (args.objectiveWeights.given()) // (likewise)
            printf("Objective weights: %s, %u of %u bins count\n", args.objectiveWeights.describe().c_str(), hipEs->objectiveWeightBins(), N / 2);
        const auto start = std::chrono::steady_clock::now();
        es->parameterMatchAudio(targetAudio.data(), (uint32_t)targetAudio.size());
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
        std::cout << "Total time to complete: " << secs << "s" << std::endl;
        const double generations = (double)hipEs->generationsRun(); // over all chunks; fewer than numGenerations each where a stop rule ended them
        const double evaluated = (double)es->population.populationLength * args.numDevices * generations;
        std::cout << "Candidates evaluated per second: " << evaluated / secs << std::endl;
        std::cout << "Chunks matched per second: " << (double)(args.hopSize ? hipEs->numChunks() : targetAudio.size() / N) / secs << std::endl;

        const uint32_t P = es->population.populationLength;
        std::vector<float> v(P * D), s(P * D), f(P);
        es->readPopulationData(v.data(), nullptr, P * D * sizeof(float), s.data(), nullptr, P * D * sizeof(float), f.data(), nullptr, P * sizeof(float));
        std::vector<float> best(v.begin(), v.begin() + D);
        if (args.returnBestEver && !hipEs->bestParametersPerChunk().empty()) { // the last chunk's best-ever individual
            best = hipEs->bestParametersPerChunk().back();
            f[0] = hipEs->bestFitnessPerChunk().back();
        }

        if (!args.matchPath.empty()) { // the parameter track, one row per chunk
            FILE *track = fopen(args.matchPath.c_str(), "w");
            if (!track) throw std::runtime_error("cannot write " + args.matchPath);
            writeMatchTrackHeader(track, D);
            const auto &rows = hipEs->bestParametersPerChunk();
            for (uint32_t c = 0; c < rows.size(); ++c)
                writeMatchTrackRow(track, c, (uint64_t)c * hipEs->hopSize(), hipEs->generationsPerChunk()[c], hipEs->bestFitnessPerChunk()[c], rows[c],
                                   es->objective.scaleParams(rows[c]));
            fclose(track);
        }
        if (args.renderMatch) { // every chunk's match, overlap-added or as one continuous voice (renderMode), on the device
            std::vector<float> whole;
            hipEs->renderMatch(whole);
            if (whole.size() > 0xFFFFFFFFull / 3) throw std::runtime_error("renderMatch: the rendering does not fit a WAV file");
            outputAudioFile(outputAudioPath, whole.data(), (uint32_t)whole.size());
            if (!args.matchReport.empty()) { // what was rendered against what was asked for, chunk by chunk, beside what the search reported
                std::vector<float> rendered;
                hipEs->scoreAgainstTargets(whole, rendered);
                FILE *report = fopen(args.matchReport.c_str(), "w");
                if (!report) throw std::runtime_error("cannot write " + args.matchReport);
                fprintf(report, "chunk,fitness,rendered_fitness\n");
                for (uint32_t c = 0; c < rendered.size(); ++c) fprintf(report, "%u,%.9g,%.9g\n", c, hipEs->bestFitnessPerChunk()[c], rendered[c]);
                fclose(report);
            }
        } else {
            // render 2^14 samples of the best match (main.cpp:270-275)
            Objective render(P, D, args.es_args.paramMin, args.es_args.paramMax, 14);
            std::vector<float> audio(1u << 14);
            synthesise(render, best, audio.data());
            outputAudioFile(outputAudioPath, audio.data(), 1u << 14);
        }

        printf("Overall best parameters found\n Fitness = %g\n", f[0]);
        const std::vector<float> scaled = es->objective.scaleParams(best);
        for (uint32_t i = 0; i < scaled.size(); ++i) printf(" p%u = %f\n", i, scaled[i]);
        return EXIT_SUCCESS;
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return EXIT_FAILURE;
    }
}
