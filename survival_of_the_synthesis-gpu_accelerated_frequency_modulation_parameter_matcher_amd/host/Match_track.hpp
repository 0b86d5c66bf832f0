// Match_track.hpp -- the hop of the chunking and the parameter track file of the sots_match driver (type.HIP.hopSize,
// type.HIP.matchPath).  Plain host code: no device, no libsots_hip (host/match_track_test.cpp runs it on a
// machine without a GPU).
#ifndef SOTS_MATCH_TRACK_HPP
#define SOTS_MATCH_TRACK_HPP

#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

// The samples between chunk starts for a hopSize as parameters.json gives it: 0 (or the key left out) is N, the
// reference's chunking; anything else must lie in ceil(N / 64) .. N - the range sots_render_overlap_add renders, at most 64
// chunks over a sample - and need not divide N.  Throws with the key's name otherwise.
inline uint32_t matchHop(double hopSize, uint32_t N)
{
    if (hopSize == 0.0) return N;
    const uint32_t lowest = (N + 63u) / 64u;
    if (!(hopSize >= (double)lowest && hopSize <= (double)N) || hopSize != (double)(uint32_t)hopSize)
        throw std::runtime_error("parameters.json: type.HIP.hopSize must be 0 or a whole number in " + std::to_string(lowest) + " .. " +
                                 std::to_string(N) + " (audio length / 64 .. audio length)");
    return (uint32_t)hopSize;
}

// chunks of N samples, hop apart, that lie wholly inside L samples: chunk i is [i hop, i hop + N).  hop = N: L / N
inline uint32_t matchChunkCount(uint64_t L, uint32_t N, uint32_t hop) { return L < N ? 0u : (uint32_t)((L - N) / hop + 1u); }

// samples the chunks cover, and the length of the overlap-add rendering of their matches
inline uint64_t matchCoveredSamples(uint32_t chunks, uint32_t N, uint32_t hop) { return chunks ? (uint64_t)(chunks - 1u) * hop + N : 0u; }

// The parameter track: chunk,start_sample,generations,fitness,u0..u{D-1},p0..p{D-1} - u the unit-range genes with %.9g,
// which gives an fp32 number back bit for bit, p the scaled parameters.
inline void writeMatchTrackHeader(FILE *f, uint32_t d)
{
    fprintf(f, "chunk,start_sample,generations,fitness");
    for (uint32_t j = 0; j < d; ++j) fprintf(f, ",u%u", j);
    for (uint32_t j = 0; j < d; ++j) fprintf(f, ",p%u", j);
    fprintf(f, "\n");
}
inline void writeMatchTrackRow(FILE *f, uint32_t chunk, uint64_t startSample, uint32_t generations, float fitness, const std::vector<float> &unit,
                               const std::vector<float> &scaled)
{
    fprintf(f, "%u,%llu,%u,%.9g", chunk, (unsigned long long)startSample, generations, (double)fitness);
    for (float u : unit) fprintf(f, ",%.9g", (double)u);
    for (float p : scaled) fprintf(f, ",%.9g", (double)p);
    fprintf(f, "\n");
}

#endif
