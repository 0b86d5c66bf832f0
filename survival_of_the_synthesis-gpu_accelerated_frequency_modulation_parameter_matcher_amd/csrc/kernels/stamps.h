// stamps.h -- the stamp buffer of the diagnostic builds (-DSOTS_STAMP, -DSOTS_STAMP_ENDS) and the macros that write it;
// empty macros in the shipped build.  A file of its own and not part of common.h: this is a device symbol of 256 KiB,
// and common.h reaches a second translation unit (sots_analyse.hip) that has no use for a copy of it.  Only
// sots_kernels.hip and the families it includes take this file.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// contraction: off (the translation unit's default; clock differences only)
#pragma clang fp contract(off)
namespace sots { namespace {

#if defined(SOTS_STAMP) || defined(SOTS_STAMP_ENDS)
// Diagnostic builds only (never the shipped library): per-wavefront shader cycles and 100 MHz
// ticks, read back with sots_debug_stamps().
__device__ unsigned long long g_stamps[2 * 16384];
#endif
#ifdef SOTS_STAMP
struct StampScope {
    unsigned long long t0, r0;
    uint32_t slot;
    __device__ StampScope(uint32_t s) : slot(s)
    {
        t0 = __builtin_amdgcn_s_memtime();
        r0 = __builtin_amdgcn_s_memrealtime();
    }
    __device__ ~StampScope()
    {
        const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
        if ((threadIdx.x & 63) == 0 && slot < 16384) {
            g_stamps[2 * slot] = t1 - t0;
            g_stamps[2 * slot + 1] = r1 - r0;
        }
    }
};
#define SOTS_STAMP_SCOPE(slot) StampScope stamp_scope_(slot)
// phase stamps of the selection kernels: shader cycles since the workgroup started, 16 phases per workgroup,
// kept behind the synthesis stamps (slots 8192..)
#define SOTS_PHASE_BEGIN() const unsigned long long phase_t0_ = __builtin_amdgcn_s_memtime()
#define SOTS_PHASE(n)                                                                                              \
    do {                                                                                                           \
        if (threadIdx.x == 0 && blockIdx.x < 512)                                                                  \
            g_stamps[2 * 8192 + blockIdx.x * 16 + (n)] = __builtin_amdgcn_s_memtime() - phase_t0_;                 \
    } while (0)
// absolute clock of any one lane (diagnostics of wavefront start skew inside a workgroup)
// the chip-wide 100 MHz clock of one lane (when workgroups start and end relative to each other)
#define SOTS_PHASE_REAL(n)                                                                                         \
    do {                                                                                                           \
        if (threadIdx.x == 0 && blockIdx.x < 512) g_stamps[2 * 8192 + blockIdx.x * 16 + (n)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#define SOTS_PHASE_ABS(n, cond)                                                                                   \
    do {                                                                                                           \
        if ((cond) && blockIdx.x < 512) g_stamps[2 * 8192 + blockIdx.x * 16 + (n)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define SOTS_STAMP_SCOPE(slot)
#define SOTS_PHASE_BEGIN()
#define SOTS_PHASE(n)
#define SOTS_PHASE_REAL(n)
#define SOTS_PHASE_ABS(n, cond)
#endif

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
