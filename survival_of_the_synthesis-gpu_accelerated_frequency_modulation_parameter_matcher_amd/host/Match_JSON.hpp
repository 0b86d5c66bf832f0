// Match_JSON.hpp -- sots_match's reading of parameters.json, apart from the driver so that it can be compiled and tested
// without the library: the minimal JSON reader and the keys whose values need checking before anything touches a device.
// Header-only, plain C++17, no HIP.
#ifndef SOTS_MATCH_JSON_HPP
#define SOTS_MATCH_JSON_HPP

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sots_hip.h" // sots_voice_graph (the struct only: nothing here calls the library)
#include "Match_track.hpp"
#include "Objective_weights.hpp"

// ---------------------------------------------------------------------------------------
// minimal JSON (objects, arrays, numbers, strings, true/false/null)
// ---------------------------------------------------------------------------------------
struct Json {
    enum Kind { Null, Bool, Number, String, Array, Object } kind = Null;
    bool b = false;
    double num = 0.0;
    std::string str;
    std::vector<Json> arr;
    std::map<std::string, Json> obj;

    const Json &operator[](const std::string &k) const
    {
        auto it = obj.find(k);
        if (kind != Object || it == obj.end()) throw std::runtime_error("parameters.json: missing key \"" + k + "\"");
        return it->second;
    }
    bool has(const std::string &k) const { return kind == Object && obj.count(k); }
    double number() const
    {
        if (kind != Number) throw std::runtime_error("parameters.json: number expected");
        return num;
    }
    std::vector<float> floats() const
    {
        std::vector<float> out;
        for (const Json &e : arr) out.push_back((float)e.number());
        return out;
    }
};

class JsonParser
{
    const std::string &s_;
    size_t i_ = 0;
    void ws()
    {
        while (i_ < s_.size() && (s_[i_] == ' ' || s_[i_] == '\n' || s_[i_] == '\t' || s_[i_] == '\r')) ++i_;
    }
    [[noreturn]] void bad(const char *what) { throw std::runtime_error(std::string("parameters.json: ") + what + " at offset " + std::to_string(i_)); }
    std::string string()
    {
        std::string out;
        ++i_;
        while (i_ < s_.size() && s_[i_] != '"') {
            if (s_[i_] == '\\' && i_ + 1 < s_.size()) ++i_;
            out.push_back(s_[i_++]);
        }
        if (i_ >= s_.size()) bad("unterminated string");
        ++i_;
        return out;
    }

public:
    explicit JsonParser(const std::string &s) : s_(s) {}
    Json value()
    {
        ws();
        if (i_ >= s_.size()) bad("unexpected end");
        Json j;
        const char c = s_[i_];
        if (c == '{') {
            j.kind = Json::Object;
            ++i_;
            ws();
            if (s_[i_] == '}') { ++i_; return j; }
            for (;;) {
                ws();
                if (s_[i_] != '"') bad("key expected");
                const std::string k = string();
                ws();
                if (s_[i_++] != ':') bad("':' expected");
                j.obj[k] = value();
                ws();
                if (s_[i_] == ',') { ++i_; continue; }
                if (s_[i_] == '}') { ++i_; return j; }
                bad("',' or '}' expected");
            }
        }
        if (c == '[') {
            j.kind = Json::Array;
            ++i_;
            ws();
            if (s_[i_] == ']') { ++i_; return j; }
            for (;;) {
                j.arr.push_back(value());
                ws();
                if (s_[i_] == ',') { ++i_; continue; }
                if (s_[i_] == ']') { ++i_; return j; }
                bad("',' or ']' expected");
            }
        }
        if (c == '"') { j.kind = Json::String; j.str = string(); return j; }
        if (s_.compare(i_, 4, "true") == 0) { j.kind = Json::Bool; j.b = true; i_ += 4; return j; }
        if (s_.compare(i_, 5, "false") == 0) { j.kind = Json::Bool; j.b = false; i_ += 5; return j; }
        if (s_.compare(i_, 4, "null") == 0) { i_ += 4; return j; }
        char *end = nullptr;
        j.num = strtod(s_.c_str() + i_, &end);
        if (end == s_.c_str() + i_) bad("value expected");
        j.kind = Json::Number;
        i_ = (size_t)(end - s_.c_str());
        return j;
    }
};

// type.HIP.objective / type.HIP.objectiveFloor (enum sots_objective, sots_set_objective): "magnitude" (0, the default: the
// reference's squared distance of the magnitudes) or "logMagnitude" (1: squared distance of ln(magnitude + objectiveFloor),
// which then must be given, 1e-30 <= objectiveFloor <= 1).  Returns whether either key was there; throws on an unknown
// name, a floor without the log objective's range, or a log objective without a floor.
inline bool readObjectiveKeys(const Json &h, uint32_t &objective, float &floor)
{
    if (!h.has("objective") && !h.has("objectiveFloor")) return false;
    uint32_t o = 0;
    if (h.has("objective")) {
        const Json &name = h["objective"];
        if (name.kind != Json::String || (name.str != "magnitude" && name.str != "logMagnitude"))
            throw std::runtime_error("parameters.json: type.HIP.objective must be \"magnitude\" or \"logMagnitude\"" +
                                     (name.kind == Json::String ? ", not \"" + name.str + "\"" : std::string()));
        o = name.str == "logMagnitude" ? 1u : 0u;
    }
    float f = 0.0f;
    if (o == 1u) {
        if (!h.has("objectiveFloor")) throw std::runtime_error("parameters.json: type.HIP.objective \"logMagnitude\" needs type.HIP.objectiveFloor");
        const double v = h["objectiveFloor"].number();
        if (!(v >= 1e-30 && v <= 1.0) || !((float)v >= 1e-30f)) // (NaN fails both; the float the library gets must be in range too)
            throw std::runtime_error("parameters.json: type.HIP.objectiveFloor must lie in 1e-30 .. 1");
        f = (float)v;
    } else if (h.has("objectiveFloor")) {
        (void)h["objectiveFloor"].number(); // a number, and ignored: the magnitude objective has no floor
    }
    objective = o;
    floor = f;
    return true;
}

// type.HIP.objectiveWeights (sots_set_objective_weights, Objective_weights.hpp): which part of the spectrum counts.
//   {"bandHz": [lo, hi]}   weight 1 on the bins with lo <= f <= hi, 0 elsewhere (0 <= lo < hi)
//   "aWeighting"           the A-curve as a power weight
//   [w_0, ..., w_{N/2-1}]  the table itself
// Returns whether the key was there.  Throws on another shape, lo >= hi, a negative or non-finite entry, all zeros; what
// depends on N and the sample rate (a band without a bin, the array's length) is makeObjectiveWeights' to refuse.
inline bool readObjectiveWeightsKey(const Json &h, Objective_Weights_Spec &spec)
{
    if (!h.has("objectiveWeights")) return false;
    const Json &v = h["objectiveWeights"];
    const std::string what = "parameters.json: type.HIP.objectiveWeights";
    Objective_Weights_Spec s;
    if (v.kind == Json::String) {
        if (v.str != "aWeighting") throw std::runtime_error(what + " must be \"aWeighting\", {\"bandHz\": [lo, hi]} or an array, not \"" + v.str + "\"");
        s.kind = Objective_Weights_Spec::AWeighting;
    } else if (v.kind == Json::Object) {
        if (!v.has("bandHz") || v.obj.size() != 1 || v["bandHz"].kind != Json::Array || v["bandHz"].arr.size() != 2)
            throw std::runtime_error(what + ": an object must be {\"bandHz\": [lo, hi]}");
        s.kind = Objective_Weights_Spec::Band;
        s.lo = v["bandHz"].arr[0].number();
        s.hi = v["bandHz"].arr[1].number();
        if (!(s.lo >= 0.0) || !(s.lo < s.hi) || !std::isfinite(s.hi)) throw std::runtime_error(what + ": bandHz needs 0 <= lo < hi");
    } else if (v.kind == Json::Array) {
        s.kind = Objective_Weights_Spec::Table;
        s.table = v.floats();
        if (s.table.empty()) throw std::runtime_error(what + ": the array is empty");
        checkObjectiveWeights(s.table, what);
    } else {
        throw std::runtime_error(what + " must be \"aWeighting\", {\"bandHz\": [lo, hi]} or an array");
    }
    spec = s;
    return true;
}

// type.HIP.hopSize (Match_track.hpp): the samples between chunk starts, 0 or absent = the audio length N.  Returns whether the
// key was there; throws - like the keys above, before any device work - on anything but 0 or a whole number in
// ceil(N / 64) .. N.
inline bool readHopSizeKey(const Json &h, uint32_t audioLength, uint32_t &hopSize)
{
    if (!h.has("hopSize")) return false;
    const Json &v = h["hopSize"];
    if (v.kind != Json::Number) throw std::runtime_error("parameters.json: type.HIP.hopSize must be a number");
    const uint32_t hop = matchHop(v.num, audioLength);
    hopSize = v.num == 0.0 ? 0u : hop;
    return true;
}

// type.HIP.renderMode: which renderer renderMatch uses.  "overlapAdd" (0, the default: sots_render_overlap_add, every chunk's
// match from phase 0, cross-faded), "continuous" (1: sots_render_continuous, one voice whose oscillators never restart, the
// parameters held from chunk centre to chunk centre) or "continuousGlide" (2: the same with the parameters interpolated
// between the centres); for the operator-graph voice "graphContinuous" (3) and "graphContinuousGlide" (4): the same two
// through sots_render_graph_continuous, and "graphFeedback" (5) and "graphFeedbackGlide" (6): the same two
// through sots_render_graph_feedback, which renders a voice with type.HIP.voiceFeedback too, and "graphGenes"
// (7) and "graphGenesGlide" (8): the same two through sots_render_graph_genes, which renders a voice with
// type.HIP.voiceFeedbackGenes too, every chunk with its own feedback indices.  Returns whether the key was there; throws -
// before any device work - on anything else.
inline bool readRenderModeKey(const Json &h, uint32_t &renderMode)
{
    if (!h.has("renderMode")) return false;
    const Json &v = h["renderMode"];
    const char *names[] = {"overlapAdd",    "continuous",         "continuousGlide", "graphContinuous", "graphContinuousGlide",
                           "graphFeedback", "graphFeedbackGlide", "graphGenes",      "graphGenesGlide"};
    if (v.kind == Json::String)
        for (uint32_t m = 0; m < 9; ++m)
            if (v.str == names[m]) return renderMode = m, true;
    throw std::runtime_error("parameters.json: type.HIP.renderMode must be \"overlapAdd\", \"continuous\" or \"continuousGlide\" (with type.HIP.synth "
                             "\"graph\": \"overlapAdd\", \"graphContinuous\" or \"graphContinuousGlide\", \"graphFeedback\" or \"graphFeedbackGlide\", "
                             "\"graphGenes\" or \"graphGenesGlide\")" +
                             (v.kind == Json::String ? ", not \"" + v.str + "\"" : std::string()));
}
// renderMode "graphContinuous" / "graphContinuousGlide" belong to the operator-graph voice, and to one without feedback
// (sots_render_graph_continuous refuses a feedback index other than 0: no scan computes that recurrence); "graphFeedback" /
// "graphFeedbackGlide" belong to the operator-graph voice, with or without feedback; "graphGenes" / "graphGenesGlide" to the
// operator-graph voice, with or without voiceFeedbackGenes.  Throws - before any device work - otherwise; the feedback is
// looked at only where the match is rendered.
inline void checkGraphRenderMode(uint32_t renderMode, bool graphVoice, bool renderMatch, const std::vector<float> &voiceFeedback)
{
    if (renderMode == 7u || renderMode == 8u) {
        if (!graphVoice)
            throw std::runtime_error("parameters.json: type.HIP.renderMode \"graphGenes\" and \"graphGenesGlide\" need type.HIP.synth \"graph\"");
        return;
    }
    if (renderMode == 5u || renderMode == 6u) {
        if (!graphVoice)
            throw std::runtime_error("parameters.json: type.HIP.renderMode \"graphFeedback\" and \"graphFeedbackGlide\" need type.HIP.synth \"graph\"");
        return;
    }
    if (renderMode != 3u && renderMode != 4u) return;
    if (!graphVoice)
        throw std::runtime_error("parameters.json: type.HIP.renderMode \"graphContinuous\" and \"graphContinuousGlide\" need type.HIP.synth \"graph\"");
    if (!renderMatch) return;
    for (float b : voiceFeedback)
        if (b != 0.0f)
            throw std::runtime_error("parameters.json: type.HIP.renderMode \"graphContinuous\" and \"graphContinuousGlide\" are not available with "
                                     "type.HIP.voiceFeedback other than 0 (\"overlapAdd\" renders such a voice, and \"graphFeedback\" renders it "
                                     "phase-continuously)");
}

// type.HIP.carryRows / type.HIP.segmentChunks (sots_batch_queue_set_carry): inside a segment of
// segmentChunks consecutive chunks a chunk starts from its predecessor's best-ever individual and rows 1..carryRows-1, beside
// fresh rows.  carryRows absent or 0: off, and segmentChunks is not looked at.  segmentChunks absent (left 0 here): the
// matcher takes ceil(chunks / chunksInFlight), one segment per slot.  Returns whether carrying is on; throws - like the keys
// above, before any device work - on carryRows that is no whole number or exceeds numParents, on segmentChunks that is no
// whole number >= 1, on carryRows without chunkQueue (only the queue carries) and on carryRows with a historyPath (that
// path matches batch by batch).
inline bool readCarryKeys(const Json &h, uint32_t numParents, uint32_t &carryRows, uint32_t &segmentChunks)
{
    if (!h.has("carryRows")) return false;
    const Json &v = h["carryRows"];
    if (v.kind != Json::Number || !(v.num >= 0.0) || v.num != std::floor(v.num))
        throw std::runtime_error("parameters.json: type.HIP.carryRows must be a whole number, 0 or more");
    if (v.num == 0.0) return false;
    if (v.num > (double)numParents)
        throw std::runtime_error("parameters.json: type.HIP.carryRows " + std::to_string((unsigned long long)std::fmin(v.num, 1.8e19)) +
                                 " exceeds evolutionary.numParents " + std::to_string(numParents) + ": only parent rows can be carried");
    if (!h.has("chunkQueue") || !h["chunkQueue"].b)
        throw std::runtime_error("parameters.json: type.HIP.carryRows needs type.HIP.chunkQueue: only the chunk queue carries rows");
    if (h.has("historyPath") && !h["historyPath"].str.empty())
        throw std::runtime_error("parameters.json: type.HIP.carryRows cannot be combined with type.HIP.historyPath: a history file is matched batch by batch");
    uint32_t segment = 0;
    if (h.has("segmentChunks")) {
        const Json &l = h["segmentChunks"];
        if (l.kind != Json::Number || !(l.num >= 1.0) || l.num != std::floor(l.num))
            throw std::runtime_error("parameters.json: type.HIP.segmentChunks must be a whole number, 1 or more");
        segment = l.num >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)l.num;
    }
    carryRows = (uint32_t)v.num;
    segmentChunks = segment;
    return true;
}

// type.HIP.deviceAnalysis / type.HIP.matchReport (sots_batch_set_analysis, sots_batch_queue_score_audio_hop).
//   deviceAnalysis  true: the chunks' target spectra are made on the device from one upload of the audio instead of chunk by
//                   chunk on the host - fp32 against fp64, so the match is not the host analysis's bit for bit.  Only the
//                   chunks in flight analyse on the device: it needs chunksInFlight > 1, one device and a population of at most
//                   1024; otherwise this throws rather than analyse on the host behind the user's back.
//   matchReport     a path: after rendering, the rendered signal is scored chunk by chunk against the stored targets and a CSV
//                   chunk,fitness,rendered_fitness is written there.  Needs renderMatch and the chunk queue (chunkQueue,
//                   chunksInFlight > 1, no historyPath: the queue keeps the targets the score reads).
// Returns whether either is on; throws - like the keys above, before any device work - where a prerequisite is missing.
inline bool readAnalysisKeys(const Json &h, uint64_t populationLength, bool &deviceAnalysis, std::string &matchReport)
{
    const bool device = h.has("deviceAnalysis") && h["deviceAnalysis"].b;
    const std::string report = h.has("matchReport") ? h["matchReport"].str : std::string();
    const bool inFlight = h.has("chunksInFlight") && h["chunksInFlight"].number() > 1.0;
    const bool oneDevice = !h.has("numDevices") || h["numDevices"].number() <= 1.0;
    if (device && !(inFlight && oneDevice && populationLength <= 1024u))
        throw std::runtime_error("parameters.json: type.HIP.deviceAnalysis needs the chunks in flight (type.HIP.chunksInFlight > 1, one device, "
                                 "a population of at most 1024): chunk by chunk the analysis stays on the host");
    if (!report.empty()) {
        if (!h.has("renderMatch") || !h["renderMatch"].b)
            throw std::runtime_error("parameters.json: type.HIP.matchReport needs type.HIP.renderMatch: it scores the rendered match");
        const bool queue = h.has("chunkQueue") && h["chunkQueue"].b && inFlight && oneDevice && populationLength <= 1024u;
        if (!queue || (h.has("historyPath") && !h["historyPath"].str.empty()))
            throw std::runtime_error("parameters.json: type.HIP.matchReport needs the chunk queue (type.HIP.chunkQueue, chunksInFlight > 1, one device, "
                                     "a population of at most 1024, no historyPath): the queue keeps the targets the score reads");
    }
    deviceAnalysis = device;
    matchReport = report;
    return device || !report.empty();
}

// type.HIP.synth "graph" with type.HIP.voiceGraph (sots_voice_graph, include/sots_hip.h): the operator-graph
// voice, e.g. {"operators": 3, "modulators": [[], [0], [1]], "carriers": [2]} - modulators[j] lists the operators that
// modulate operator j, carriers the operators that are heard.  Returns whether the voice is the graph; throws - like the keys
// above, before any device work - where one key comes without the other, on a shape that is not the one above, on
// numDimensions other than 2 x operators, and on renderMode "continuous" / "continuousGlide" with renderMatch (that
// phase-continuous renderer is written per fixed voice; "graphContinuous" / "graphContinuousGlide" are the graph voice's).  Whether the topology is a valid one is the library's rule
// (csrc/sots_rules.h), which sots_create_graph applies before it touches a device.
inline bool readVoiceGraphKeys(const Json &h, uint32_t numDimensions, bool renderMatch, uint32_t renderMode, sots_voice_graph &graph)
{
    const bool named = h.has("synth") && h["synth"].kind == Json::String && h["synth"].str == "graph";
    const std::string what = "parameters.json: type.HIP.voiceGraph";
    if (!named && !h.has("voiceGraph")) return false;
    if (!named) throw std::runtime_error(what + " needs type.HIP.synth \"graph\"");
    if (!h.has("voiceGraph")) throw std::runtime_error("parameters.json: type.HIP.synth \"graph\" needs type.HIP.voiceGraph");
    const Json &v = h["voiceGraph"];
    const char *shape = " must be {\"operators\": n, \"modulators\": [[...], ...], \"carriers\": [...]}";
    if (v.kind != Json::Object || !v.has("operators") || !v.has("modulators") || !v.has("carriers") || v.obj.size() != 3 ||
        v["operators"].kind != Json::Number || v["modulators"].kind != Json::Array || v["carriers"].kind != Json::Array)
        throw std::runtime_error(what + shape);
    // an operator index as a mask bit; one that no mask holds becomes bit 31, which the library's rule names
    auto mask = [&](const Json &list) {
        if (list.kind != Json::Array) throw std::runtime_error(what + shape);
        uint32_t m = 0;
        for (const Json &e : list.arr) {
            if (e.kind != Json::Number || !(e.num >= 0.0) || e.num != std::floor(e.num))
                throw std::runtime_error(what + ": operator indices are whole numbers, 0 or more");
            m |= 1u << (e.num < 31.0 ? (uint32_t)e.num : 31u);
        }
        return m;
    };
    const double ops = v["operators"].num;
    if (!(ops >= 0.0) || ops != std::floor(ops)) throw std::runtime_error(what + ": operators must be a whole number");
    sots_voice_graph g{};
    g.struct_size = sizeof g;
    g.num_operators = ops >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)ops;
    if (v["modulators"].arr.size() != (size_t)ops || ops > 8.0)
        throw std::runtime_error(what + ": modulators needs one list per operator (" + std::to_string(v["modulators"].arr.size()) + " lists, " +
                                 std::to_string((unsigned long long)std::fmin(ops, 1.8e19)) + " operators, at most 8)");
    for (size_t j = 0; j < v["modulators"].arr.size(); ++j) g.modulators[j] = mask(v["modulators"].arr[j]);
    g.carriers = mask(v["carriers"]);
    if (numDimensions != 2u * g.num_operators && !h.has("voiceFeedbackGenes")) // (with that key: readVoiceFeedbackGenesKey counts the genes)
        throw std::runtime_error("parameters.json: evolutionary.numDimensions " + std::to_string(numDimensions) + " must be 2 x type.HIP.voiceGraph.operators = " +
                                 std::to_string(2u * g.num_operators));
    if (renderMatch && (renderMode == 1u || renderMode == 2u))
        throw std::runtime_error("parameters.json: type.HIP.renderMode \"continuous\" and \"continuousGlide\" are not available with type.HIP.synth \"graph\"");
    graph = g;
    return true;
}

// type.HIP.voiceWaveforms (sots_set_voice_waveforms, include/sots_hip.h): the graph voice's operator
// waveforms, one name per operator - "sine", "half", "abs", "pulse", "even", "absEven", "square", "saw" - a key of its own
// beside voiceGraph.  Returns whether the key is there; codes receives SOTS_WAVE_* per operator.  Throws - before any device
// work - without type.HIP.synth "graph", on anything but a list of `operators` strings, and on a name that is no waveform.
inline bool readVoiceWaveformsKey(const Json &h, bool graphVoice, uint32_t operators, std::vector<uint32_t> &codes)
{
    if (!h.has("voiceWaveforms")) return false;
    const std::string what = "parameters.json: type.HIP.voiceWaveforms";
    if (!graphVoice) throw std::runtime_error(what + " needs type.HIP.synth \"graph\"");
    const Json &v = h["voiceWaveforms"];
    if (v.kind != Json::Array || v.arr.size() != operators)
        throw std::runtime_error(what + " needs one name per operator (" + (v.kind == Json::Array ? std::to_string(v.arr.size()) + " names" : std::string("not a list")) +
                                 ", " + std::to_string(operators) + " operators)");
    static const char *const names[8] = {"sine", "half", "abs", "pulse", "even", "absEven", "square", "saw"};
    std::vector<uint32_t> out;
    for (const Json &e : v.arr) {
        uint32_t w = 0;
        while (w < 8 && !(e.kind == Json::String && e.str == names[w])) ++w;
        if (w == 8)
            throw std::runtime_error(what + ": " + (e.kind == Json::String ? "\"" + e.str + "\"" : std::string("an entry that is no string")) +
                                     " is no waveform (sine, half, abs, pulse, even, absEven, square, saw)");
        out.push_back(w);
    }
    codes = out;
    return true;
}

// type.HIP.voiceFeedback (sots_set_voice_feedback, include/sots_hip.h): the graph voice's per-operator
// feedback indices, one number in [0, 2] per operator, a key of its own beside voiceGraph.  Returns whether the key is there.
// Throws - before any device work - without type.HIP.synth "graph", on anything but a list of `operators` numbers, and on a
// number outside [0, 2].
inline bool readVoiceFeedbackKey(const Json &h, bool graphVoice, uint32_t operators, std::vector<float> &index)
{
    if (!h.has("voiceFeedback")) return false;
    const std::string what = "parameters.json: type.HIP.voiceFeedback";
    if (!graphVoice) throw std::runtime_error(what + " needs type.HIP.synth \"graph\"");
    const Json &v = h["voiceFeedback"];
    if (v.kind != Json::Array || v.arr.size() != operators)
        throw std::runtime_error(what + " needs one number per operator (" + (v.kind == Json::Array ? std::to_string(v.arr.size()) + " numbers" : std::string("not a list")) +
                                 ", " + std::to_string(operators) + " operators)");
    std::vector<float> out;
    for (const Json &e : v.arr) {
        if (e.kind != Json::Number) throw std::runtime_error(what + ": an entry that is no number");
        if (!(e.num >= 0.0 && e.num <= 2.0)) throw std::runtime_error(what + ": " + std::to_string(e.num) + " is outside 0..2");
        const float b = (float)e.num; // (decided on the double: a number beyond fp32 never reaches the conversion)
        out.push_back(b == 0.0f ? 0.0f : b);
    }
    index = out;
    return true;
}

// type.HIP.voiceFeedbackGenes (sots_create_graph_genes, include/sots_hip.h): one 0 or 1 per operator, like
// voiceFeedback; 1 makes that operator's feedback index a gene of the individual - evolutionary.numDimensions is then
// 2 x operators + the number of 1s, and paramMins / paramMaxs hold that many entries, the genes' ranges (within [0, 2]) behind
// the others.  Returns whether the key is there; mask receives bit j for operator j.  Throws - before any device work -
// without type.HIP.synth "graph", on anything but a list of `operators` entries that are 0 or 1, on an operator that also has
// a voiceFeedback other than 0, on more than 16 genes, on numDimensions / paramMins / paramMaxs that do not count the genes,
// and on the renderModes "graphContinuous" to "graphFeedbackGlide" (those renderers take the index from the voice, not from
// the row; "overlapAdd" renders every row with its own, and so do "graphGenes" / "graphGenesGlide", phase-continuously).  The
// ranges themselves are the library's rule.
inline bool readVoiceFeedbackGenesKey(const Json &h, bool graphVoice, uint32_t operators, const std::vector<float> &voiceFeedback, uint32_t numDimensions,
                                      size_t numParamMins, size_t numParamMaxs, uint32_t renderMode, uint32_t &mask)
{
    if (!h.has("voiceFeedbackGenes")) return false;
    const std::string what = "parameters.json: type.HIP.voiceFeedbackGenes";
    if (!graphVoice) throw std::runtime_error(what + " needs type.HIP.synth \"graph\"");
    const Json &v = h["voiceFeedbackGenes"];
    if (v.kind != Json::Array || v.arr.size() != operators)
        throw std::runtime_error(what + " needs one 0 or 1 per operator (" + (v.kind == Json::Array ? std::to_string(v.arr.size()) + " entries" : std::string("not a list")) +
                                 ", " + std::to_string(operators) + " operators)");
    uint32_t m = 0, genes = 0;
    for (size_t j = 0; j < v.arr.size(); ++j) {
        const Json &e = v.arr[j];
        if (e.kind != Json::Number || (e.num != 0.0 && e.num != 1.0)) throw std::runtime_error(what + ": an entry that is neither 0 nor 1");
        if (e.num == 0.0) continue;
        if (j < voiceFeedback.size() && voiceFeedback[j] != 0.0f)
            throw std::runtime_error(what + ": operator " + std::to_string(j) + " also has a type.HIP.voiceFeedback of " + std::to_string(voiceFeedback[j]) +
                                     " (one or the other)");
        m |= 1u << j;
        ++genes;
    }
    const uint32_t d = 2u * operators + genes;
    const std::string count = ": " + std::to_string(operators) + " operators and " + std::to_string(genes) + " feedback genes ";
    if (d > 16u) throw std::runtime_error(what + count + "are " + std::to_string(d) + " genes, more than 16");
    if (numDimensions != d || numParamMins != d || numParamMaxs != d)
        throw std::runtime_error(what + count + "need numDimensions " + std::to_string(d) + " with " + std::to_string(d) + " paramMins and paramMaxs, got " +
                                 std::to_string(numDimensions) + ", " + std::to_string(numParamMins) + " and " + std::to_string(numParamMaxs));
    static const char *const modes[] = {"", "", "", "graphContinuous", "graphContinuousGlide", "graphFeedback", "graphFeedbackGlide"};
    if (m && renderMode >= 3u && renderMode <= 6u)
        throw std::runtime_error(what + ": every row has its own feedback index, which type.HIP.renderMode \"" + modes[renderMode] + "\" cannot render (\"overlapAdd\" does, and \"graphGenes\" renders it phase-continuously)");
    mask = m;
    return true;
}

// type.HIP.graphSynthForm (sots_set_graph_synth_form, include/sots_hip.h): which synthesis kernel the graph
// voice runs, "auto" (the default), "lanes" or "timeParallel" - the same audio bit for bit.  Returns whether the key is
// there.  Throws - before any device work - without type.HIP.synth "graph" and on any other value.
inline bool readGraphSynthFormKey(const Json &h, bool graphVoice, uint32_t &form)
{
    if (!h.has("graphSynthForm")) return false;
    const std::string what = "parameters.json: type.HIP.graphSynthForm";
    if (!graphVoice) throw std::runtime_error(what + " needs type.HIP.synth \"graph\"");
    const Json &v = h["graphSynthForm"];
    const std::string s = v.kind == Json::String ? v.str : std::string();
    if (s == "auto") form = SOTS_GRAPH_FORM_AUTO;
    else if (s == "lanes") form = SOTS_GRAPH_FORM_LANES;
    else if (s == "timeParallel") form = SOTS_GRAPH_FORM_TIME_PARALLEL;
    else throw std::runtime_error(what + " must be \"auto\", \"lanes\" or \"timeParallel\"");
    return true;
}

#endif
