// graph_feedback_host.cpp -- the host's own graph synthesiser with per-operator feedback (host/Evolutionary_Strategy.hpp:
// Objective::synthesiseAudioGraph with codes and indices), driven for tests/test_graph_feedback_cpu.py: the case file holds,
// as 32-bit words, log2 N, the operator count, the carriers, eight modulator masks, eight codes, the row count, eight
// feedback indices as floats (a first index of NaN: the overload without indices), sixteen minima and sixteen maxima as
// floats, then the rows' unit-range genes; the audio goes to the output file row after row.  CPU only: no GPU, no libsots_hip.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd/host/Evolutionary_Strategy.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    uint32_t head[20];
    float beta[8], range[32];
    if (fread(head, 4, 20, in) != 20 || fread(beta, 4, 8, in) != 8 || fread(range, 4, 32, in) != 32) return 2;
    const uint32_t log2n = head[0], ops = head[1], carriers = head[2], rows = head[19];
    const uint32_t *mods = head + 3, *codes = head + 11;
    if (log2n > 15 || ops < 2 || ops > 8 || rows > 4096) return 2;
    std::vector<float> genes((size_t)rows * 2 * ops);
    if (fread(genes.data(), 4, genes.size(), in) != genes.size()) return 2;
    fclose(in);
    Objective obj(rows, 2 * ops, std::vector<float>(range, range + 2 * ops), std::vector<float>(range + 16, range + 16 + 2 * ops), log2n);
    std::vector<float> audio(1u << log2n);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    for (uint32_t r = 0; r < rows; ++r) {
        const std::vector<float> row(genes.begin() + (size_t)r * 2 * ops, genes.begin() + (size_t)(r + 1) * 2 * ops);
        if (std::isnan(beta[0])) obj.synthesiseAudioGraph(ops, carriers, mods, codes, row, audio.data());
        else obj.synthesiseAudioGraph(ops, carriers, mods, codes, beta, row, audio.data());
        fwrite(audio.data(), 4, audio.size(), out);
    }
    fclose(out);
    return 0;
}
