// Objective_weights.hpp -- per-bin weight tables of the spectral objective (sots_set_objective_weights): which part of the
// spectrum matters.  With weights w_k the fitness is F = sum_k w_k e_k^2 over the bins k = 0 .. N/2-1, e_k the signed error
// of the objective in force; bin k lies at f_k = k sampleRate / N.  Header-only, plain C++17, no HIP and no library: what
// type.HIP.objectiveWeights names (Match_JSON.hpp) becomes a table here, and everything that can be wrong with it is
// found here, before anything touches a device.
#ifndef SOTS_OBJECTIVE_WEIGHTS_HPP
#define SOTS_OBJECTIVE_WEIGHTS_HPP

#include <cmath>
#include <cstdint>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

struct Objective_Weights_Spec {
    // None: every bin counts alike (no table is set).  Band: w = 1 for lo <= f_k <= hi, else 0.  AWeighting: the A-curve as
    // a power weight, w_k = 10^(A(f_k) / 10), w_0 = 0.  Table: N/2 numbers taken as given.
    enum Kind { None, Band, AWeighting, Table } kind = None;
    double lo = 0.0, hi = 0.0; // Band, in Hz
    std::vector<float> table;  // Table

    bool given() const { return kind != None; }
    std::string describe() const
    {
        std::ostringstream s;
        if (kind == Band) s << "bandHz " << lo << " .. " << hi;
        else if (kind == AWeighting) s << "aWeighting";
        else if (kind == Table) s << "table of " << table.size() << " bins";
        else s << "none";
        return s.str();
    }
};

// A(f) in dB (IEC 61672): 20 log10 R_A(f) + 2.00 with
// R_A(f) = 12194^2 f^4 / ((f^2 + 20.6^2) sqrt((f^2 + 107.7^2)(f^2 + 737.9^2)) (f^2 + 12194^2)); -infinity at f = 0
inline double aWeightingDb(double f)
{
    const double f2 = f * f;
    const double ra = 12194.0 * 12194.0 * f2 * f2 /
                      ((f2 + 20.6 * 20.6) * std::sqrt((f2 + 107.7 * 107.7) * (f2 + 737.9 * 737.9)) * (f2 + 12194.0 * 12194.0));
    return 20.0 * std::log10(ra) + 2.00;
}
// the power weight of a bin at f Hz under the A-curve: 10^(A(f) / 10), 0 at f = 0
inline double aWeightingPower(double f) { return f > 0.0 ? std::pow(10.0, aWeightingDb(f) / 10.0) : 0.0; }

// what the library accepts: finite, >= 0, not all zero (throws with `what` in front otherwise)
inline void checkObjectiveWeights(const std::vector<float> &w, const std::string &what)
{
    bool any = false;
    for (size_t k = 0; k < w.size(); ++k) {
        if (!(w[k] >= 0.0f) || !std::isfinite(w[k]))
            throw std::runtime_error(what + ": entry " + std::to_string(k) + " must be finite and not negative");
        any = any || w[k] > 0.0f;
    }
    if (!any) throw std::runtime_error(what + ": at least one weight must be positive");
}

// the table of N/2 weights for rows of N samples at sampleRate; empty for Kind::None.  Throws on 0 <= lo < hi violated,
// a band that holds no bin, a table of another length, a negative or non-finite entry, all zeros.
inline std::vector<float> makeObjectiveWeights(const Objective_Weights_Spec &spec, uint32_t N, double sampleRate)
{
    const std::string what = "objectiveWeights";
    const uint32_t half = N / 2;
    std::vector<float> w;
    if (spec.kind == Objective_Weights_Spec::None) return w;
    if (spec.kind == Objective_Weights_Spec::Band) {
        if (!(spec.lo >= 0.0) || !(spec.lo < spec.hi) || !std::isfinite(spec.hi))
            throw std::runtime_error(what + ": bandHz needs 0 <= lo < hi");
        w.assign(half, 0.0f);
        uint32_t inside = 0;
        for (uint32_t k = 0; k < half; ++k) {
            const double f = (double)k * sampleRate / (double)N;
            if (spec.lo <= f && f <= spec.hi) w[k] = 1.0f, ++inside;
        }
        if (inside == 0) throw std::runtime_error(what + ": bandHz holds no bin of the " + std::to_string(half) + " (bin spacing " + std::to_string(sampleRate / N) + " Hz)");
        return w;
    }
    if (spec.kind == Objective_Weights_Spec::AWeighting) {
        w.resize(half);
        for (uint32_t k = 0; k < half; ++k) w[k] = (float)aWeightingPower((double)k * sampleRate / (double)N);
    } else {
        if (spec.table.size() != half)
            throw std::runtime_error(what + ": the array needs " + std::to_string(half) + " entries (N/2), got " + std::to_string(spec.table.size()));
        w = spec.table;
    }
    checkObjectiveWeights(w, what);
    return w;
}

#endif
