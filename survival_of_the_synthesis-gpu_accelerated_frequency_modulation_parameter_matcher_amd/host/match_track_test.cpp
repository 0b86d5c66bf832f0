// match_track_test.cpp -- CPU-only checks of Match_track.hpp and the hopSize key (no GPU, no libsots_hip): prints what
// tests/test_render_cpu.py compares - the hop a hopSize gives or the refusal's text, the chunk count formula, and a
// parameter track whose u columns must give the fp32 bits back.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "Match_JSON.hpp"
#include "Match_track.hpp"

int main(int argc, char **argv)
{
    // ---- hopSize through the JSON key: "hop <text> -> <hopSize> <samples between chunks>" or "-> refused: <text>" ----
    const uint32_t N = 1024;
    const char *texts[] = {"{}", "{\"hopSize\": 0}", "{\"hopSize\": 1024}", "{\"hopSize\": 512}", "{\"hopSize\": 101}", "{\"hopSize\": 16}",
                           "{\"hopSize\": 15}", "{\"hopSize\": 1025}", "{\"hopSize\": -512}", "{\"hopSize\": 100.5}", "{\"hopSize\": \"512\"}",
                           "{\"hopSize\": 1e99}", "{\"hopSize\": true}"};
    for (const char *t : texts) {
        try {
            const Json h = JsonParser(t).value();
            uint32_t hopSize = 0;
            const bool given = readHopSizeKey(h, N, hopSize);
            printf("hop %s -> given %d hopSize %u hop %u\n", t, (int)given, hopSize, matchHop((double)hopSize, N));
        } catch (const std::exception &e) {
            printf("hop %s -> refused: %s\n", t, e.what());
        }
    }
    // an audio length that is no multiple of 64: the lowest hop is rounded up
    for (double hs : {3.0, 4.0, 5.0}) {
        try {
            printf("hop200 %g -> %u\n", hs, matchHop(hs, 200));
        } catch (const std::exception &e) {
            printf("hop200 %g -> refused\n", hs);
        }
    }

    // ---- chunk count and covered length: "chunks L N hop count covered" ----
    const uint64_t lengths[] = {0, 1023, 1024, 1025, 1535, 1536, 2048, 3072, 5 * 1024 + 7, 44100};
    for (uint64_t L : lengths)
        for (uint32_t hop : {1024u, 512u, 101u, 16u}) {
            const uint32_t c = matchChunkCount(L, N, hop);
            printf("chunks %llu %u %u %u %llu\n", (unsigned long long)L, N, hop, c, (unsigned long long)matchCoveredSamples(c, N, hop));
        }

    // ---- the parameter track: rows of fp32 bit patterns given on the command line (hex), written to argv[1] ----
    if (argc > 2) {
        FILE *f = fopen(argv[1], "w");
        if (!f) return 1;
        const uint32_t d = 4;
        writeMatchTrackHeader(f, d);
        std::vector<float> u, p;
        uint32_t row = 0;
        for (int i = 2; i < argc; ++i) {
            const uint32_t b = (uint32_t)strtoul(argv[i], nullptr, 16);
            float v;
            memcpy(&v, &b, 4);
            u.push_back(v);
            p.push_back(v * 3520.0f);
            if (u.size() == d) {
                writeMatchTrackRow(f, row, (uint64_t)row * 512u, 20u + row, u[0], u, p);
                ++row;
                u.clear(), p.clear();
            }
        }
        fclose(f);
    }
    return 0;
}
