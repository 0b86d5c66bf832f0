"""An independent model of variation (recombine_source, mutate_gene, make_gene of csrc/kernels/variation.h), NumPy only.

recombine() is written as the reference words it (ocl_program.cl:130-137), as a scatter in 64-bit integers: gene g of local
individual l of block b GOES TO local individual (l + g (b + 1)) mod B, and block b copies parent block b mod
max(1, floor(parents / B)).  The kernel is the gather of the same permutation, with shifts and masks or with divisions; the
C oracle is a loop.  Neither is called here.

mutate() takes the 13 random words of every gene (oracle.mutate_words: the generator itself is pinned by
tests/test_oracle.py).  The coin, the twelve adds, the division, the candidate value, the reflect test and the second
candidate are order-fixed fp32 operations, done here in np.float32 in the kernel's written order: values must equal the
device's bit for bit.  The new step is computed in fp64 from the fp32 inputs, s alpha^(+-sqrt(1/D)) exp(|g| - c)^(1/D) with
c the fp32 root_two_over_pi and g the fp32 gauss after the reflect decision: the device's expf / powf, its fp32 constants
and its two fp32 multiplies are judged against it by step_ratio().
"""
import numpy as np

F32 = np.float32
ALPHA = F32(1.4)
ROOT_TWO_OVER_PI = np.sqrt(F32(2.0) / F32(np.pi))  # sqrtf(2.f / (float)M_PI), Evolutionary_Strategy.hpp:611-627
assert ROOT_TWO_OVER_PI.dtype == np.float32

# |s_dev - s_64| <= STEP_RTOL |s_64| + STEP_ATOL: the project's figure for this stage (tests/test_gpu_parity.py), taken
# against fp64, and one subnormal spacing for a result that rounds into the subnormals
STEP_RTOL = 2e-6
STEP_ATOL = 2.0 ** -149
# fp32 products at or above this round to +inf (round to nearest even): FLT_MAX + half an ulp
F32_OVERFLOW = 2.0 ** 128 - 2.0 ** 103


def recombine(v, s, parents, block):
    """(values, steps) of the recombined population, for any block that divides P"""
    v, s = np.ascontiguousarray(v, F32), np.ascontiguousarray(s, F32)
    p, d = v.shape
    assert block >= 1 and p % block == 0
    npb = max(1, parents // block)
    b = np.arange(p // block, dtype=np.uint64)[:, None, None]
    l = np.arange(block, dtype=np.uint64)[None, :, None]
    g = np.arange(d, dtype=np.uint64)[None, None, :]
    B = np.uint64(block)
    dst = (b * B + (l + g * (b + np.uint64(1))) % B).astype(np.int64)
    src = np.broadcast_to(((b % np.uint64(npb)) * B + l).astype(np.int64), dst.shape)
    col = np.broadcast_to(g, dst.shape).astype(np.int64)
    vo, so = np.full_like(v, np.nan), np.full_like(s, np.nan)
    vo[dst, col] = v[src, col]
    so[dst, col] = s[src, col]
    # a scatter must hit every place exactly once
    hit = np.zeros((p, d), np.int64)
    np.add.at(hit, (dst, col), 1)
    assert np.all(hit == 1)
    return vo, so


def draw_unit(words):
    """(float)((int)word) / 2147483647.0f, ocl_program.cl:27,61"""
    return np.ascontiguousarray(words, np.uint32).view(np.int32).astype(F32) / F32(2147483647.0)


def mutate(v, s, words, d, detail=False):
    """(values fp32, steps fp64) after mutation; words[..., 13] uint32 per gene.  detail: also a dict of the branch masks"""
    v, s = np.ascontiguousarray(v, F32), np.ascontiguousarray(s, F32)
    words = np.ascontiguousarray(words, np.uint32)
    assert words.shape == v.shape + (13,) and s.shape == v.shape
    with np.errstate(all="ignore"):
        even = (words[..., 0] % np.uint32(2)) == 0
        ek = np.where(even, ALPHA, F32(1.0) / ALPHA).astype(F32)
        total = np.zeros(v.shape, F32)
        for t in range(1, 13):
            total = total + draw_unit(words[..., t])
        gauss = total / F32(12.0)
        first = v + ek * s * gauss
        reflect = (first < F32(0.0)) | (first > F32(1.0))       # false for NaN, as in C
        gauss = np.where(reflect, gauss * F32(-0.5), gauss).astype(F32)
        second = v + ek * s * gauss
        new_v = np.where(reflect, second, first).astype(F32)
        assert new_v.dtype == np.float32 and gauss.dtype == np.float32
        sign = np.where(even, 1.0, -1.0)
        factor = np.float64(ALPHA) ** (sign * np.sqrt(1.0 / d)) * np.exp(np.abs(gauss.astype(np.float64)) - np.float64(ROOT_TWO_OVER_PI)) ** (1.0 / d)
        new_s = s.astype(np.float64) * factor
    if detail:
        outside = (second < F32(0.0)) | (second > F32(1.0))
        return new_v, new_s, {"even": even, "reflect": reflect, "still_outside": reflect & outside}
    return new_v, new_s


def survivors(v0, s0, v1, s1, k):
    """rows < k of the varied population (v1, s1) are bit copies of the sorted one's (v0, s0)"""
    v1, s1 = np.array(v1, copy=True), np.array(s1, copy=True)
    v1[:k], s1[:k] = v0[:k], s0[:k]
    return v1, s1


def generation(v, s, parents, block, words, k=0):
    """make_gene over a sorted population: recombine, mutate, survivors.  (values fp32, steps fp64)"""
    d = np.shape(v)[1]
    rv, rs = recombine(v, s, parents, block)
    mv, ms = mutate(rv, rs, words, d)
    return survivors(np.asarray(v, F32), np.asarray(s, F32).astype(np.float64), mv, ms, k)


def init(words):
    """initPopulation (ocl_program.cl:56-65) from one word per gene: (values, steps)"""
    u = draw_unit(words)
    return np.where(u < F32(0.0), -u, u).astype(F32), np.full(u.shape, 0.1, F32)


def step_ratio(s_dev, s64):
    """per gene, |s_dev - s_64| / (STEP_RTOL |s_64| + STEP_ATOL); 0 where the device has exactly what IEEE arithmetic
    leaves no choice about, inf where it does not:
      * a model step of 0, +-inf or NaN (from a step of 0, inf or NaN: the factor is finite and positive) must be 0, that
        inf or a NaN on the device too (NaN payloads are not compared);
      * a device step of +-inf for a finite model step is right only where a value within the bound of the model's rounds
        to inf in fp32 (|s_64| (1 + STEP_RTOL) >= FLT_MAX + ulp/2); a finite device step is held to the bound as ever."""
    s_dev = np.asarray(s_dev, F32).astype(np.float64)
    s64 = np.asarray(s64, np.float64)
    with np.errstate(all="ignore"):
        ratio = np.abs(s_dev - s64) / (STEP_RTOL * np.abs(s64) + STEP_ATOL)
        exact = np.isnan(s64) | np.isinf(s64) | (s64 == 0.0)
        same = (np.isnan(s64) & np.isnan(s_dev)) | (s_dev == s64)
        ratio = np.where(exact, np.where(same, 0.0, np.inf), ratio)
        overflow = ~exact & np.isinf(s_dev)
        may = (np.abs(s64) * (1.0 + STEP_RTOL) >= F32_OVERFLOW) & (np.sign(s_dev) == np.sign(s64))
        ratio = np.where(overflow, np.where(may, 0.0, np.inf), ratio)
    return np.where(np.isnan(ratio), np.inf, ratio)


def same_values(a, b):
    """bit for bit, except that a NaN matches any NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---- the populations the GPU tests write ------------------------------------------------------------------------------------
EDGE_STEPS = np.array([0.0, 2.0 ** -149, 2.0 ** -130, 2.0 ** -126, 1e-30, 1e-6, 0.1, 3.0, 1e30, 3e38, np.inf, np.nan], F32)
EDGE_VALUES = np.array([0.0, 2.0 ** -149, 0.5, 1.0 - 2.0 ** -24, 1.0, -0.3, 1.7, np.nan], F32)
EDGE_ROWS = 4096


def edge_population(d, finite=False, rows=EDGE_ROWS):
    """every step of EDGE_STEPS crossed with every value of EDGE_VALUES, each pair in every gene column many times, in a
    seeded order.  finite: the part a synthesis kernel may be handed - steps in [0, 3], finite values (inside [-0.3, 1.7])"""
    steps, values = EDGE_STEPS, EDGE_VALUES
    if finite:
        steps = steps[np.isfinite(steps) & (steps <= 3.0)]
        values = values[np.isfinite(values)]
    pairs = steps.size * values.size
    rng = np.random.default_rng(0xED6E + d + (1000 if finite else 0))
    pick = np.stack([rng.permutation(np.arange(rows) % pairs) for _ in range(d)], axis=1)  # per column: every pair rows / pairs times
    return values[pick % values.size].copy(), steps[pick // values.size].copy()


SITE_STEPS = np.array([0.02, 0.5, 3.0], F32)


def site_population(p, d, seed):
    """values uniform in [0, 1), steps 0.02, 0.5 or 3.0: small enough for a synthesis kernel, large enough that the reflect
    branch is taken often and its second candidate is often still outside the unit interval"""
    rng = np.random.default_rng(seed)
    return rng.random((p, d), dtype=F32), SITE_STEPS[rng.integers(0, SITE_STEPS.size, (p, d))].copy()


def coverage(v, s, words, d):
    """shares over the mutated genes: (coin even, coin odd, reflect taken, reflect not taken, still outside / reflected)"""
    _, _, m = mutate(v, s, words, d, detail=True)
    n = m["even"].size
    taken = int(np.count_nonzero(m["reflect"]))
    return (np.count_nonzero(m["even"]) / n, np.count_nonzero(~m["even"]) / n, taken / n, 1.0 - taken / n,
            np.count_nonzero(m["still_outside"]) / max(1, taken))


# ---- the cases of tests/test_gpu_variation.py (here, so that tests/test_variation_cpu.py can judge them without a GPU) ---------
SEED = 0x5EED0001
N_LOG2 = 8            # N = 256 throughout: rows are cheap
SITE_GENERATION = 3   # the Philox generation counter of the site cases
SITE_BLOCK, SITE_PARENTS = 24, 80   # 3 parent blocks (no power of two); breeding rows 72 < 80 parents

# (a) recombination geometries: (voice, parents, offspring, block).  Blocks 3, 24, 48, 96, 100 and B = P; parents below,
# equal to and not a multiple of the block; 3, 5 and 9 parent blocks; the last one wraps k_recombine's grid-stride loop
# (99 984 x 12 genes on at most 2048 workgroups of 256)
GEOMETRIES = [
    (0, 9, 291, 3), (1, 72, 216, 24), (2, 120, 168, 24), (3, 216, 264, 24), (0, 20, 268, 24), (1, 24, 264, 24), (2, 100, 188, 24),
    (3, 48, 240, 48), (0, 150, 234, 48), (1, 96, 288, 96), (2, 300, 276, 96), (3, 100, 300, 100), (0, 520, 380, 100),
    (1, 77, 223, 300), (2, 64, 512, 576), (3, 96, 96, 32), (2, 72, 99912, 24)]

# (b) every site of make_gene inside a context's generation loop, by the smallest shape that selects it on 256 CUs:
# (site, voice, population, does the synthesis kernel make the individuals?).  share = ceil(P / 256).
SITES = [
    # synth_time_parallel: share <= 16 / 12 / 5 / 9 for the 2-op / 3-op / triple / 4-op voice -> k_synth_tp, and the fuse rule folds
    ("k_synth_tp<2op>", 0, 768, True), ("k_synth_tp<3op>", 1, 768, True), ("k_synth_tp<triple>", 2, 768, True), ("k_synth_tp<4op>", 3, 768, True),
    # triple voice, share 6 > 5: not time-parallel, 12 genes: no clause of the fuse rule holds -> k_recombine_mutate
    ("k_recombine_mutate<triple>", 2, 1536, False),
    # 4-op voice, share 10 > 9 and <= 64: 8 genes > 6, no operators in lanes -> k_recombine_mutate (its cut helper form
    # k_synth<4op, 1, true, 2, 3> is selected only where the fuse rule is forced, which the shipped build cannot be)
    ("k_recombine_mutate<4op>", 3, 2328, False),
    # 2-op voice, share 17 > 16: d <= 6 and P <= 128 x 256 fold; waves = 1, cut -> k_synth<2op, 1, true>
    ("k_synth<2op,1,help> 1 wave", 0, 4104, True),
    # ... share 65: waves = 2, cut -> k_synth<2op, 1, true> with two wavefronts per stage
    ("k_synth<2op,1,help> 2 waves", 0, 16392, True),
    # 3-op voice, share 13 > 12 and <= 64: waves = 1 -> k_synth<3op, 1, true, 2>  (from share 65 synth_operators_in_lanes
    # takes the 3-op voice, so k_synth<3op, 2, true> is selected by no shape on 256 CUs)
    ("k_synth<3op,1,help,2>", 1, 3096, True),
    # synth_operators_in_lanes: 3-op at share 65 ... 240, 4-op from share 65 -> k_synth_ol
    ("k_synth_ol<3op>", 1, 16392, True), ("k_synth_ol<4op>", 3, 16392, True),
    # 2-op voice, d <= 4 and P >= 192 x 256: share 192, waves = 3, not cut, one tile per workgroup -> k_synth<2op, 0, true>
    ("k_synth<2op,0,help>", 0, 49152, True),
]
SITE_SURVIVORS = (0, 1, SITE_PARENTS)

# (e) counters
WRAP_P = 768                              # the counter cases' population (2-op voice, block 24, 80 parents)
WRAP_GID = (1 << 32) - WRAP_P // 2        # gid_base + i wraps in the middle of the population
EDGE_GENERATIONS = (0xFFFFFFFF, 0x80000000)
EDGE_CHUNK = 0xFFFFFFFF
BATCH_FIRST_CHUNK, BATCH_CHUNKS = 0xFFFFFFFE, 4
