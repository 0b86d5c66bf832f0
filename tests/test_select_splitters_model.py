"""NumPy model of the one-launch selection (k_sel_splitters): every key is ranked between stored 64-bit
splitters, and the positions are exact WHATEVER the splitters are.  No GPU: this pins the invariants the kernel is
written to - the sanitised splitters make disjoint buckets that cover every key, a key's position is the number of
keys below its bucket plus its rank inside it, the keys at a fixed rank step are the next splitters, and the float
compare the kernel streams with decides exactly what the 64-bit compare decides."""
import numpy as np
import pytest

from test_gpu_parity import fitness_pattern

PATTERNS = ["random", "ascending", "descending", "constant", "few_values", "tile_skew", "converged", "clones", "specials"]
SPLITTER_KINDS = ["fresh", "stale", "constant", "zero", "ones", "descending", "nan_region", "garbage"]
BITS_NEG_INF, BITS_POS_INF, BITS_NAN = 0x007FFFFF, 0xFF800000, 0xFFFFFFFD


def order_bits(f):
    f = np.asarray(f, np.float32)
    u = np.where(f == 0, np.float32(0), f).view(np.uint32).astype(np.uint64)
    u = np.where(u & np.uint64(0x80000000), ~u & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    return np.where(np.isnan(f), np.uint64(BITS_NAN), u)


def make_keys(f):
    return (order_bits(f) << np.uint64(32)) | np.arange(len(f), dtype=np.uint64)


def sanitise(slot):
    t = np.array(slot, np.uint64)
    t[0] = 0
    return np.maximum.accumulate(t)


def normalise(t):
    """the least key >= t that compares like t against every key that exists (spl_normalise)"""
    b = int(t) >> 32
    if b < BITS_NEG_INF:
        return BITS_NEG_INF << 32
    if b == 0x7FFFFFFF:
        return 0x80000000 << 32
    return int(t)


def bound_float(t):
    b = int(t) >> 32
    u = (b ^ 0x80000000) if b & 0x80000000 else (~b & 0xFFFFFFFF)
    return np.array([u], np.uint32).view(np.float32)[0]


def rank_step(need, B):
    """positions q * step, q < B, reach 1.25 * need: the next generation's cut must fall in front of the last splitter"""
    return (need * 5 // 4 + B - 2) // (B - 1)


def model_select(f, slot, step, need):
    """positions of every key (perm[position] = row) and the next slot, bucket by bucket as the workgroups do.  The open
    last bucket, when no row below `need` falls into it, is not ordered: the splitters whose positions it holds become
    its own lower bound (any key may be a splitter; the model orders it all the same, to check every position)"""
    keys = make_keys(f)
    B, P = len(slot), len(f)
    t = sanitise(slot)
    perm = np.full(P, -1, np.int64)
    nxt = np.zeros(B, np.uint64)
    owned = np.zeros(P, np.int64)
    sizes = []
    for j in range(B):
        lo = t[j]
        inside = keys >= lo
        if j + 1 < B:
            inside &= keys < t[j + 1]
        c = int(np.sum(keys < lo))
        bucket = np.sort(keys[inside])
        owned[inside] += 1
        sizes.append(len(bucket))
        pos = c + np.arange(len(bucket))
        assert np.all(perm[pos] == -1)
        perm[pos] = (bucket & np.uint64(0xFFFFFFFF)).astype(np.int64)
        q = pos // step
        take = (pos % step == 0) & (q >= 1) & (q < B)
        if j + 1 == B and c >= need:
            nxt[-(-c // step):] = lo
        else:
            nxt[q[take]] = bucket[take]
    assert np.all(owned == 1), "the buckets must be disjoint and cover every key"
    return perm, nxt, sizes


def splitters(kind, B, P, step, f, rng):
    if kind == "fresh":       # the same population's own order at the rank step
        k = np.sort(make_keys(f))
        s = k[np.arange(B) * step]
    elif kind == "stale":     # another population's
        k = np.sort(make_keys(fitness_pattern("tile_skew" if rng.random() < 0.5 else "converged", P, rng)))
        s = k[np.arange(B) * step]
    elif kind == "constant":
        s = np.full(B, make_keys(f)[P // 3], np.uint64)
    elif kind == "zero":
        s = np.zeros(B, np.uint64)
    elif kind == "ones":
        s = np.full(B, 0xFFFFFFFFFFFFFFFF, np.uint64)
    elif kind == "descending":
        s = np.sort(make_keys(f))[np.arange(B) * step][::-1].copy()
    elif kind == "nan_region":  # bounds among and above the NaN keys
        s = (np.uint64(BITS_NAN) << np.uint64(32)) | rng.integers(0, P, B).astype(np.uint64)
        s[B // 2:] += np.uint64(1 << 32)
    else:                       # garbage: any 64 bits
        s = rng.integers(0, 1 << 63, B, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, B).astype(np.uint64)
    return s.astype(np.uint64)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", SPLITTER_KINDS)
def test_positions_are_exact_for_any_splitters(O, pattern, kind):
    P, B, need = 4096, 64, 1024
    step = rank_step(need, B)
    rng = np.random.default_rng(len(pattern) * 31 + len(kind))
    f = fitness_pattern(pattern, P, rng)
    slot = splitters(kind, B, P, step, f, rng)
    perm, nxt, sizes = model_select(f, slot, step, need)
    assert np.array_equal(perm, O.sort_perm(f))
    # the next slot: the keys at the rank step, ascending as written, up to where the open bucket began (if the cut was in
    # front of it: from there on its lower bound)
    want = np.sort(make_keys(f))[np.arange(B) * step]
    open_from = P - sizes[-1]
    exact = np.arange(B) * step < open_from if open_from >= need else np.ones(B, bool)
    exact[0] = False
    assert np.array_equal(nxt[exact], want[exact]) and np.all(nxt[~exact][1:] == sanitise(slot)[-1])
    # ... and fed back, they make buckets of at most `step` keys below the last splitter, and the same positions
    perm2, nxt2, sizes2 = model_select(f, nxt, step, need)
    assert np.array_equal(perm2, perm) and max(sizes2[:-1]) <= step
    if kind == "fresh":
        assert np.array_equal(nxt2, nxt), "a population selected twice keeps its slot"
    if kind in ("zero", "ones", "constant"):
        assert max(sizes) > P // 2, "one workgroup owns more than half of the keys: the slow path"


@pytest.mark.parametrize("pattern", PATTERNS)
def test_float_compare_equals_key_compare(pattern):
    """key < bound, decided as the stream decides it for bounds with the bits of numbers: fitness < bound's float, the
    row index only where they are equal; NaN compares false, -0 equals +0"""
    P = 2048
    rng = np.random.default_rng(7 + len(pattern))
    f = fitness_pattern(pattern, P, rng)
    f[5], f[6] = -0.0, 0.0
    keys = make_keys(f)
    idx = np.arange(P, dtype=np.uint64)
    bounds = list(rng.choice(keys, 24)) + [0, 1 << 32, 0x7FFFFFFF << 32 | 9, 0x80000000 << 32 | 6, BITS_NEG_INF << 32 | 3,
                                           BITS_POS_INF << 32 | 100, 0x00000001 << 32, make_keys(np.float32([-np.inf]))[0]]
    checked = 0
    for t in bounds:
        n = normalise(t)
        assert np.array_equal(keys < np.uint64(n), keys < np.uint64(t)), "normalising a bound moved a key across it"
        if (n >> 32) > BITS_POS_INF:
            continue  # the kernel compares such bounds as 64-bit keys
        bf = bound_float(n)
        with np.errstate(invalid="ignore"):
            below = (f < bf) | ((f == bf) & (idx < np.uint64(n & 0xFFFFFFFF)))
        assert np.array_equal(below, keys < np.uint64(n))
        checked += 1
    assert checked >= 8
