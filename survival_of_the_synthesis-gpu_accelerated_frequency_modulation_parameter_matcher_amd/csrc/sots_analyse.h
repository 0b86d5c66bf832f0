// sots_analyse.h -- analysis of a signal on the device (sots_analyse.hip): the magnitude spectra of
// overlapping frames from ONE uploaded buffer, and the per-frame score of such spectra against stored targets.
// Internal to libsots_hip.so; the public boundary is sots_batch_set_analysis, sots_batch_analyse_audio_hop and
// sots_batch_queue_score_audio_hop in include/sots_hip.h.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "sots_kernels.h" // Objective

namespace sots {

// Frame f = signal[f hop, f hop + N), read in place: no copy of the frames is made.  The caller sees to it that `signal`
// holds (frames - 1) hop + N floats; no lane loads beyond them.  Per frame: window (the engine's fp32 table), real-input
// FFT in fp32 with the engine's twiddle table, and for k < N/2 the bin scaled BEFORE its magnitude is taken,
//     x_k = X_k * (inv_n * inv_wf),   m_k = sqrt(re(x_k)^2 + im(x_k)^2).
// bins == false: out[f N/2 + k] = m_k (floats).  bins == true: out holds the x_k themselves, N/2 float2 per frame - what
// launch_score_frames reads.  A frame's bits depend on its N samples alone: not on hop, frames, or where the frame starts.
hipError_t launch_analyse(hipStream_t st, const float *signal, const float *window, const float2 *twiddle, float *out, bool bins,
                          uint32_t log2n, uint32_t hop, uint32_t frames, float inv_n, float inv_wf);

// fitness[f] = sum_k (u_k e_k)^2 over the N/2 bins of frame f, e_k = bin_error (kernels/objective.h) of x_k against
// targets[f N/2 + k] with scale 1: the magnitude is the m_k above bit for bit, so a frame scored against targets that
// launch_analyse made of the same samples gives exactly 0 under either objective.  Under the log objective `targets` holds
// ln(t + floor) (launch_objective_map); with weights obj.weights is u[N/2].  The sum has a fixed order: lane l adds its
// bins l, l + 64, ... in ascending order, then the wavefront's 64 sums are added as wave_sum adds them.
hipError_t launch_score_frames(hipStream_t st, const float2 *bins, const float *targets, float *fitness, uint32_t log2n, uint32_t frames,
                               const Objective &obj);

// Device memory of the analysis, owned by a batch: allocated on first use, grown when a call needs more, freed with the
// batch.  signal: the uploaded samples; out: magnitudes or bins; fitness: one float per frame.
struct AnalyseScratch {
    float *signal = nullptr, *out = nullptr, *fitness = nullptr;
    size_t signal_floats = 0, out_floats = 0, fitness_floats = 0;
};
hipError_t analyse_reserve(AnalyseScratch &as, size_t signal_floats, size_t out_floats, size_t fitness_floats);
void analyse_release(AnalyseScratch &as);

} // namespace sots
