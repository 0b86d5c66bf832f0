// fft.h -- complex helpers, the radix-2/4/8 butterflies, Stockham passes, fft_forward and the real-input split of the
// wavefront-per-row transform; k_fft_x and k_fft_big use the complex helpers too.
#pragma once
#include "common.h"

// contraction: on (see below: the transform is bit-matched to nothing, fused multiply-adds are allowed here)
#pragma clang fp contract(on)
namespace sots { namespace {

// ------------------------------------------------------------------------------------
// Batched real FFT (replaces clFFT, Evolutionary_Strategy_OpenCL.hpp:156-192,555-561)
// and fitnessPopulation (ocl_program.cl:594-659 with the CPU bin range k < N/2,
// Evolutionary_Strategy_CPU.hpp:235).
//
// One wavefront transforms one individual: the N real samples are read as M = N/2 complex
// points, E = M/64 per lane, and go through Stockham autosort passes of radix 8 or 4 (three
// or two radix-2 butterfly layers done in registers), exchanging through a padded LDS
// buffer between passes.  A final split step turns Z[k], Z[M-k] into the real-input bins
// X[k], X[M-k].
// ------------------------------------------------------------------------------------
// The transform is not bit-matched to anything (the oracle's FFT is fp64), so fused
// multiply-adds are allowed here and only here; "on" contracts within one expression, which
// keeps k_fft<.,1> and k_fitness on identical arithmetic.
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 cmul(float2 a, float2 b)
{
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// ---- complex values as 2-vectors (register pairs): v_pk_add/mul/fma_f32 do a complex add, or half a complex
// multiply, per instruction, and every wave64 vector instruction holds the SIMD for 4 cycles whatever it does
__device__ __forceinline__ v2f_t xv(float2 a) { return v2f_t{a.x, a.y}; }
// a * w: (a.x, a.y) * w.x + (-a.y, a.x) * w.y - a packed multiply and a packed fma (operand selects and negations are
// instruction modifiers)
// The packed instructions select the low or high half of each source per result half (op_sel, op_sel_hi) and negate
// per half (neg_lo, neg_hi); the compiler uses the selects but flips signs of single halves with v_xor and copies, so
// the few shapes the transform needs are written out.
__device__ __forceinline__ v2f_t xc_mul(v2f_t a, v2f_t w)
{
    // both halves in ONE statement: around a statement the compiler pads wait states it cannot rule out (s_nop; a statement
    // per instruction, rounds 2-3: profiles/r04_experiments.md)
    v2f_t t;
    asm("v_pk_mul_f32 %1, %0, %2 op_sel:[0,0] op_sel_hi:[1,0]\n\t"                                              // (a.x w.x, a.y w.x)
        "v_pk_fma_f32 %0, %0, %2, %1 op_sel:[1,1,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0]" : "+v"(a), "=&v"(t) : "v"(w)); // (-a.y w.y, a.x w.y) + t
    return a;
}
__device__ __forceinline__ v2f_t xc_mul_neg_i(v2f_t a) { return v2f_t{a.y, -a.x}; }
// (-i a) * w = (a.y w.x + a.x w.y, a.y w.y - a.x w.x)
__device__ __forceinline__ v2f_t xc_mul_negi_w(v2f_t a, v2f_t w)
{
    v2f_t t;
    asm("v_pk_mul_f32 %1, %0, %2 op_sel:[1,0] op_sel_hi:[0,0] neg_hi:[1,0]\n\t"                                  // (a.y w.x, -a.x w.x)
        "v_pk_fma_f32 %0, %0, %2, %1 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "+v"(a), "=&v"(t) : "v"(w));               // (a.x w.y, a.y w.y) + t
    return a;
}
// a + conj(b), a - conj(b)
__device__ __forceinline__ v2f_t xc_add_conj(v2f_t a, v2f_t b)
{
    v2f_t r;
    asm("v_pk_add_f32 %0, %1, %2 neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ v2f_t xc_sub_conj(v2f_t a, v2f_t b)
{
    v2f_t r;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}


// a * e^{-i pi/4} and a * e^{-3 i pi/4} for a = (x, y): ((x + y) s, (y - x) s) and ((y - x) s, -(x + y) s), s = sqrt(1/2) -
// one packed add with swapped and negated halves and one packed multiply each (the same sums and products as the scalar
// form, so the same bits)
__device__ __forceinline__ float2 rot_m45(float2 a)
{
    const v2f_t av = xv(a);
    v2f_t t;
    asm("v_pk_add_f32 %0, %1, %1 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(t) : "v"(av)); // (x + y, y - x)
    t = t * v2f_t{0.70710678118654752440f, 0.70710678118654752440f};
    return make_float2(t.x, t.y);
}
__device__ __forceinline__ float2 rot_m135(float2 a)
{
    const v2f_t av = xv(a);
    v2f_t t;
    asm("v_pk_add_f32 %0, %1, %1 op_sel:[1,0] op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[1,1]" : "=v"(t) : "v"(av)); // (y - x, -x - y)
    t = t * v2f_t{0.70710678118654752440f, 0.70710678118654752440f};
    return make_float2(t.x, t.y);
}

// a + (-i) d = (a.x + d.y, a.y - d.x) and a - (-i) d = (a.x - d.y, a.y + d.x) in ONE packed add each (half selects and negations
// are instruction modifiers): a butterfly's rotation by -i never becomes a register shuffle
__device__ __forceinline__ float2 add_negi(float2 a, float2 d)
{
    v2f_t r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(xv(a)), "v"(xv(d)));
    return make_float2(r.x, r.y);
}
__device__ __forceinline__ float2 sub_negi(float2 a, float2 d)
{
    v2f_t r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0] neg_lo:[0,1]" : "=v"(r) : "v"(xv(a)), "v"(xv(d)));
    return make_float2(r.x, r.y);
}

template <int R> struct Dft;
template <> struct Dft<2> {
    static __device__ __forceinline__ void run(float2 *v)
    {
        const float2 a = v[0], b = v[1];
        v[0] = cadd(a, b);
        v[1] = csub(a, b);
    }
};
template <> struct Dft<4> {
    static __device__ __forceinline__ void run(float2 *v)
    {
        const float2 t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]);
        const float2 t2 = cadd(v[1], v[3]), d = csub(v[1], v[3]);
        v[0] = cadd(t0, t2);
        v[1] = add_negi(t1, d); // t1 + (-i) d
        v[2] = csub(t0, t2);
        v[3] = sub_negi(t1, d);
    }
};
template <> struct Dft<8> {
    static __device__ __forceinline__ void run(float2 *v)
    {
        float2 e[4] = {v[0], v[2], v[4], v[6]};
        float2 o[4] = {v[1], v[3], v[5], v[7]};
        Dft<4>::run(e);
        Dft<4>::run(o);
        // o[k] *= exp(-2 pi i k / 8); k = 2 (a rotation by -i) folded into its butterfly
        o[1] = rot_m45(o[1]);
        o[3] = rot_m135(o[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = k == 2 ? add_negi(e[k], o[k]) : cadd(e[k], o[k]);
            v[k + 4] = k == 2 ? sub_negi(e[k], o[k]) : csub(e[k], o[k]);
        }
    }
};

// LDS index padding: one extra complex slot per 8 keeps the stride-8 / stride-64 writes of
// the first two passes and the unit-stride reads off each other's banks.
__device__ __forceinline__ int lds_pad(int i) { return i + (i >> 3); }

// One Stockham pass of radix R with NS = product of the radices already applied.
// Register slot s holds element lane + 64 s of the pass input; butterfly b uses slots
// b + t*(E/R), t < R.  Output element t of butterfly j goes to (j-k)*R + k + t*NS with
// k = j mod NS.  The twiddles e^{-2 pi i t k / (NS R)} depend only on the lane, so they are
// loop-invariant per kernel: twr (when non-null) holds them in registers, B*(R-1) values in
// (b, t) order; otherwise they come from the N-entry table e^{-2 pi i q / N}, N = 2M.
template <int M, int R, int NS>
__device__ __forceinline__ void load_pass_twiddles(float2 *twr, const float2 *__restrict__ tw, int lane)
{
    constexpr int E = M / kWave, B = E / R, stride = (2 * M) / (NS * R);
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const int k = (lane + kWave * b) & (NS - 1);
#pragma unroll
        for (int t = 1; t < R; ++t) twr[b * (R - 1) + t - 1] = tw[t * k * stride];
    }
}

// LAST: the pass's outputs stay in registers instead of going to LDS.  For the last pass
// (NS * R == M, so k == j and j0 == j) output t of butterfly b is element lane + 64 (b + B t): slot
// b + B t of x, i.e. afterwards x[s] = Z[lane + 64 s].
template <int M, int R, int NS, bool LAST = false>
__device__ __forceinline__ void fft_pass(float2 (&x)[M / kWave], float2 *__restrict__ lds,
                                         const float2 *__restrict__ tw, const float2 *twr, int lane)
{
    constexpr int E = M / kWave, B = E / R;
    static_assert(!LAST || NS * R == M, "only the final pass can stay in registers");
    float2 out[LAST ? E : 1];
    static_assert(E % R == 0, "radix must divide the per-lane element count");
#pragma unroll
    for (int b = 0; b < B; ++b) {
        const int j = lane + kWave * b;
        const int k = j & (NS - 1);
        float2 v[R];
#pragma unroll
        for (int t = 0; t < R; ++t) v[t] = x[b + t * B];
        if constexpr (NS > 1) {
            constexpr int stride = (2 * M) / (NS * R);
#pragma unroll
            for (int t = 1; t < R; ++t) v[t] = cmul(v[t], twr ? twr[b * (R - 1) + t - 1] : tw[t * k * stride]);
        }
        Dft<R>::run(v);
        if constexpr (LAST) {
#pragma unroll
            for (int t = 0; t < R; ++t) out[b + t * B] = v[t];
        } else {
            const int j0 = (j - k) * R + k;
#pragma unroll
            for (int t = 0; t < R; ++t) lds[lds_pad(j0 + t * NS)] = v[t];
        }
    }
    if constexpr (LAST) {
#pragma unroll
        for (int sl = 0; sl < E; ++sl) x[sl] = out[sl];
    }
}

template <int M>
__device__ __forceinline__ void lds_reload(float2 (&x)[M / kWave], const float2 *__restrict__ lds, int lane)
{
#pragma unroll
    for (int s = 0; s < M / kWave; ++s) x[s] = lds[lds_pad(lane + kWave * s)];
}

// First pass (NS = 1, no twiddles) straight from the 16-byte loads of the row.  Lane l holds
// the float4 = two complex points at pair index l + 64 h, i.e. complex elements
// e0 = 2l + 128 h and e0 + 1.  With element e = j + (M/R) t:
//   B = E/R >= 2: the lane already owns every t of butterflies j = 2l + 64 bb (+1), bb even;
//   B == 1      : lanes l and l+32 hold the even-t and odd-t halves of butterflies 2l, 2l+1;
//                 one v_permlane32_swap per register gives lane l all of 2l and lane l+32
//                 all of 2l+1.
template <int M, int R>
__device__ __forceinline__ void fft_first_pass(const float4 (&q)[M / kWave / 2], float2 *__restrict__ lds, int lane)
{
    constexpr int E = M / kWave;
    static_assert(E == R, "one first-pass butterfly per lane (N = 512: radix 4, N = 1024: radix 8)");
    float2 v[R];
#pragma unroll
    for (int h = 0; h < R / 2; ++h) {
        const auto sx = __builtin_amdgcn_permlane32_swap(__float_as_uint(q[h].x), __float_as_uint(q[h].z), false, false);
        const auto sy = __builtin_amdgcn_permlane32_swap(__float_as_uint(q[h].y), __float_as_uint(q[h].w), false, false);
        v[2 * h] = make_float2(__uint_as_float(sx[0]), __uint_as_float(sy[0]));
        v[2 * h + 1] = make_float2(__uint_as_float(sx[1]), __uint_as_float(sy[1]));
    }
    Dft<R>::run(v);
    const int j = 2 * (lane & 31) + (lane >> 5);
#pragma unroll
    for (int t = 0; t < R; ++t) lds[lds_pad(j * R + t)] = v[t];
}

// All passes for M complex points (N = 512: 4.4.4.4, N = 1024: 8.8.8), starting from the row as
// loaded; the last pass stays in registers: x[s] = Z[lane + 64 s].  The per-lane pass twiddles
// (all passes after the first) are loop-invariant and live in registers.
template <int M> constexpr int tw_count() { return M == 256 ? 9 : 14; }

template <int M>
__device__ __forceinline__ void preload_twiddles(float2 (&twr)[tw_count<M>()], const float2 *__restrict__ tw, int lane)
{
    static_assert(M == 256 || M == 512, "wavefront-per-row FFT is for N <= 1024");
    if constexpr (M == 256) {
        load_pass_twiddles<M, 4, 4>(&twr[0], tw, lane);
        load_pass_twiddles<M, 4, 16>(&twr[3], tw, lane);
        load_pass_twiddles<M, 4, 64>(&twr[6], tw, lane);
    } else {
        load_pass_twiddles<M, 8, 8>(&twr[0], tw, lane);
        load_pass_twiddles<M, 8, 64>(&twr[7], tw, lane);
    }
}

// Between the passes of ONE wavefront's transform.  A workgroup of one wavefront: __syncthreads(), of which the compiler
// drops the s_barrier and keeps the fence (s_waitcnt lgkmcnt(0)).  A workgroup of several wavefronts, each with its own
// piece of LDS (W > 1 below): the fence written out - a barrier would tie the wavefronts together for nothing.  (The LDS
// executes a wavefront's instructions in order; ordering them by a compiler barrier alone measures the same,
// profiles/r03_experiments.md.)
template <bool ALONE>
__device__ __forceinline__ void wave_lds_sync()
{
    if constexpr (ALONE) __syncthreads();
    else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

template <int M, bool ALONE = true>
__device__ __forceinline__ void fft_forward(const float4 (&q)[M / kWave / 2], float2 *__restrict__ lds,
                                            const float2 *__restrict__ tw, const float2 (&twr)[tw_count<M>()], int lane,
                                            float2 (&x)[M / kWave])
{
#define SOTS_SYNC() wave_lds_sync<ALONE>()
#define SOTS_FIRST(R)                        \
    fft_first_pass<M, R>(q, lds, lane);      \
    SOTS_SYNC();
#define SOTS_PASS(R, NS, OFF)                             \
    fft_pass<M, R, NS>(x, lds, tw, &twr[OFF], lane);      \
    SOTS_SYNC();
#define SOTS_NEXT()                          \
    lds_reload<M>(x, lds, lane);             \
    SOTS_SYNC();
#define SOTS_LAST(R, NS, OFF) fft_pass<M, R, NS, true>(x, lds, tw, &twr[OFF], lane);
    if constexpr (M == 256) {
        SOTS_FIRST(4) SOTS_NEXT() SOTS_PASS(4, 4, 0) SOTS_NEXT() SOTS_PASS(4, 16, 3) SOTS_NEXT() SOTS_LAST(4, 64, 6)
    } else {
        SOTS_FIRST(8) SOTS_NEXT() SOTS_PASS(8, 8, 0) SOTS_NEXT() SOTS_LAST(8, 64, 7)
    }
#undef SOTS_SYNC
#undef SOTS_FIRST
#undef SOTS_PASS
#undef SOTS_NEXT
#undef SOTS_LAST
}

// Real-input split for the pair (k, M-k), 0 <= k < M/2:
//   Ee = (Z[k] + conj Z[M-k]) / 2,  Oo = -i (Z[k] - conj Z[M-k]) / 2,  T = e^{-2 pi i k/N} Oo
//   X[k] = Ee + T,  X[M-k] = conj(Ee - T)
// With Z[M] read as Z[0] the same formula gives X[0] = Re Z0 + Im Z0 and the Nyquist bin
// X[M] = Re Z0 - Im Z0 for k = 0, so no lane takes a different path.  Bin M/2, which no pair
// covers, is X[M/2] = conj Z[M/2].
// After the last pass lane l holds z[s] = Z[l + 64 s].  For k = l + 64 q the partner
// Z[M-k] = Z[(64-l) + 64 (E-1-q)] is slot E-1-q of lane 64-l: one ds_bpermute per dword through
// the LDS crossbar, no LDS memory and no bank conflicts (this replaces a write of the whole
// transform to LDS and two reads of it).  Lane 0 pairs with itself one slot further:
// Z[M - 64 q] = its own slot E-q, and Z[M] = Z[0] for q = 0.
template <int M>
__device__ __forceinline__ float2 split_partner(const float2 (&z)[M / kWave], int q, int lane, int partner_addr)
{
    constexpr int E = M / kWave;
    const float2 mine = z[q == 0 ? 0 : E - q];                    // what lane 0 needs
    const float2 send = z[E - 1 - q];                             // what lane 64-l needs from this lane
    const float px = __int_as_float(__builtin_amdgcn_ds_bpermute(partner_addr, __float_as_int(send.x)));
    const float py = __int_as_float(__builtin_amdgcn_ds_bpermute(partner_addr, __float_as_int(send.y)));
    return lane == 0 ? mine : make_float2(px, py);
}

// In packed form, without the two 1/2 factors: 2 X[k] and 2 conj X[M-k] (a factor of two is exact in fp32; the fitness
// folds it into its magnitude scale and takes magnitudes, the spectrum writer halves and conjugates as it stores) - six
// packed instructions for two bins
__device__ __forceinline__ void split_pair_2x(float2 a, float2 bz, float2 w, v2f_t &xa2, v2f_t &xbc2)
{
    const v2f_t av = xv(a), bv = xv(bz);
    const v2f_t ee = xc_add_conj(av, bv), dd = xc_sub_conj(av, bv);
    const v2f_t t = xc_mul_negi_w(dd, xv(w));
    xa2 = ee + t;
    xbc2 = ee - t;
}

}} // namespace sots::(anonymous)

#pragma clang fp contract(off)
