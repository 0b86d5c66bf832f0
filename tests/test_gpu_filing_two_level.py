"""The two-level key filing (kernels/sel_keys.h, kBktTwoLevel: the lookup of every launch over at most 65 536 rows) on
the GPU, at the smallest populations that take the twelve-wavefront spectral kernel: P = 3072, 4096 = 1024 + 3072 and
the odd 3200, 2-op, N = 1024.  What sots_stage_bucket_fitness files - read back as it lies in device memory - equals a
NumPy model of "bucket of a key = number of bounds at or below it, minus one" exactly, whatever the slot holds; the rows
a list-mode selection then places (SORT_TOP_ONLY) are the full sort's (SORT_FULL) first S rows bit for bit; the flat
lookup of a launch over more than 65 536 rows names the same bucket for every key; the fused loop equals the staged one."""
import numpy as np
import pytest

from test_gpu_parity import make_pair, target_audio
from test_gpu_select_splitters import prime
from test_select_lists_model import bucket_of
from test_select_splitters_model import make_keys, normalise

pytestmark = pytest.mark.gpu

SIZES = [(768, 2304), (1024, 3072), (800, 2400)]   # P = 3072 (the smallest wide launch), 4096, 3200 (no multiple of 64 x 4)
SHARDS, SEG = 16, 128
PATTERNS = ["random", "specials", "constant"]


def fitness(pattern, P, rng):
    if pattern == "constant":       # every key ties: the row index decides
        return np.full(P, 0.25, np.float32)
    f = rng.random(P, dtype=np.float32)
    if pattern == "specials":
        for value in (np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5):
            f[rng.choice(P, P // 24, replace=False)] = value
    return f


def model_buckets(keys, slot):
    """number of bounds at or below the key, minus one: t_0 = 0, the running maximum of the slot, normalised"""
    t = np.array(slot, np.uint64)
    t[0] = 0
    t = np.array([normalise(x) for x in np.maximum.accumulate(t)], np.uint64)
    j = np.searchsorted(t, keys, side="right").astype(np.int64) - 1
    assert np.array_equal(j, bucket_of(keys, slot))     # (the statement of tests/test_select_lists_model.py)
    return j


def check_lists(f, slot, counts, lists, rows=None):
    """counts[B, 16], lists[B, 16, 128] against the model: every key of a closed bucket counted in the segment of its
    wavefront (64 consecutive rows, in turn), stored while the segment has places; nothing in the open bucket"""
    B = len(slot)
    keys = make_keys(f)
    j = model_buckets(keys, slot)
    rows = len(f) if rows is None else rows     # (the keys from `rows` on are padding and must all be open)
    assert np.all(j[rows:] == B - 1)
    closed = np.flatnonzero(j[:rows] < B - 1)
    seg = j[closed] * SHARDS + (closed // 64) % SHARDS
    want = np.bincount(seg, minlength=B * SHARDS).reshape(B, SHARDS)
    assert np.array_equal(counts, want), "counters differ from the model"
    assert not counts[B - 1].any()
    order = np.lexsort((keys[closed], seg))
    seg_sorted, keys_sorted = seg[order], keys[closed][order]
    starts = np.searchsorted(seg_sorted, np.arange(B * SHARDS + 1))
    flat = lists.reshape(B * SHARDS, SEG)
    for s in np.flatnonzero(want.reshape(-1)):
        expect = keys_sorted[starts[s]:starts[s + 1]]
        got = np.sort(flat[s, :min(len(expect), SEG)])
        if len(expect) <= SEG:
            assert np.array_equal(got, expect), f"bucket {s // SHARDS} segment {s % SHARDS}"
        else:   # an overflowed segment keeps the first 128 arrivals: distinct keys of this segment
            assert len(np.unique(got)) == SEG and np.all(np.isin(got, expect)), f"bucket {s // SHARDS} segment {s % SHARDS} (overflowed)"
    return j


def slots(pkg, es, f, rng):
    """name, slot: what the issue of the two-level filing lists"""
    B = es.select_splitter_count()
    P = len(f)
    k = np.sort(make_keys(f))
    prime(pkg, es, fitness("random", P, rng))
    yield "previous selection", es.read_select_splitters()
    yield "all equal", np.full(B, k[P // 2], np.uint64)
    occur = k[np.arange(B) * (P // B)].copy()          # bounds that ARE keys of the population
    yield "keys that occur", occur
    wide = occur.copy()
    wide[-1] = k[(B - 1) * (P // B) - 1] | np.uint64(0x80000000)   # a last bound that is no key: bit 31 of its low word set
    yield "last bound bit 31", wide
    yield "random 64-bit", rng.integers(0, 1 << 63, B, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, B, dtype=np.uint64)
    yield "ones", np.full(B, 0xFFFFFFFFFFFFFFFF, np.uint64)
    yield "zero", np.zeros(B, np.uint64)


@pytest.fixture(scope="module", params=SIZES, ids=lambda c: f"P{c[0] + c[1]}")
def ctx(request, pkg, O):
    parents, offspring = request.param
    es, _ = make_pair(pkg, O, parents, offspring, 0, 10)
    es.set_select_plan(pkg.capi.SELECT_SPLITTERS)
    yield es, parents
    es.close()


@pytest.mark.parametrize("pattern", PATTERNS)
def test_filed_lists_equal_the_model_and_selection_equals_full_sort(pkg, O, ctx, pattern):
    es, parents = ctx
    P, D = es.P, es.D
    S = max(parents, max(1, parents // 32) * 32)
    rng = np.random.default_rng(30 * P + len(pattern))
    f = fitness(pattern, P, rng)
    v = rng.random((P, D), dtype=np.float32)
    s = rng.random((P, D), dtype=np.float32)
    # the reference, once: the full sort on the device, itself the oracle's stable order
    es.set_sort_mode(pkg.capi.SORT_FULL)
    es.write_population(v, s, f)
    es.select(); es.rotate()
    full = es.read_population()
    perm = O.sort_perm(f)
    assert np.array_equal(full[0], v[perm]) and np.array_equal(full[1], s[perm]) and np.array_equal(full[2], f[perm], equal_nan=True)
    names = []
    for name, slot in slots(pkg, es, f, rng):
        names.append(name)
        es.set_sort_mode(pkg.capi.SORT_TOP_ONLY)
        es.write_population(v, s, f)
        es.write_select_splitters(slot)
        es.bucket_fitness()
        counts, lists = es.read_select_lists()
        check_lists(f, slot, counts, lists)
        es.select(); es.rotate()
        got = es.read_population()
        for x, y in zip(got, full):
            assert np.array_equal(x[:S], y[:S], equal_nan=True), f"slot '{name}': selected rows differ from the full sort's"
    assert len(names) == 7


def test_both_lookups_name_the_same_bucket_for_every_key(pkg, O):
    """one population at P = 4096 through the staged bucket kernel with the two-level lookup, and the same keys - padded
    with NaN rows, which sort last - through a launch over 131 072 rows, the size rule's other branch: today's lookup"""
    small, _ = make_pair(pkg, O, 1024, 3072, 0, 10)
    big, _ = make_pair(pkg, O, 32768, 98304, 0, 10)
    rng = np.random.default_rng(4096)
    P, B = small.P, small.select_splitter_count()
    assert big.select_splitter_count() == B
    f = fitness("specials", P, rng)
    f[np.isnan(f)] = 2.0        # (NaN is the padding's alone here)
    f[::5] = f[3]               # ties across bounds: the row index decides
    k = np.sort(make_keys(f))
    fb = np.full(big.P, np.nan, np.float32)
    fb[:P] = f
    for slot in (k[np.arange(B) * (P // B)].copy(), k[np.arange(B) * 3].copy(),
                 rng.integers(0, 1 << 63, B, dtype=np.uint64) * np.uint64(2) + np.uint64(1)):
        slot = np.minimum(slot, np.uint64((0xFFFFFFFD << 32) - 1))  # every padding key above every bound: open
        got = []
        for es, fit in ((small, f), (big, fb)):
            es.set_select_plan(pkg.capi.SELECT_SPLITTERS)
            z = np.zeros((es.P, es.D), np.float32)
            es.write_population(z, z, fit)
            es.write_select_splitters(slot)
            es.bucket_fitness()
            counts, lists = es.read_select_lists()
            check_lists(fit, slot, counts, lists, rows=P)
            got.append((counts, lists))
        assert np.array_equal(got[0][0], got[1][0]), "the two lookups count differently"
        # (an overflowed segment keeps whichever 128 keys arrived first: both were checked against the model above)
        filled = np.arange(SEG)[None, None, :] < np.where(got[0][0] <= SEG, got[0][0], 0)[:, :, None]
        assert filled.any()
        a, b = (np.sort(np.where(filled, x[1], np.uint64(0)), axis=2) for x in got)
        assert np.array_equal(a, b), "the two lookups file a key under different buckets"
    small.close(); big.close()


def test_fused_loop_equals_staged_loop_6_generations(pkg, O):
    a, _ = make_pair(pkg, O, 1024, 3072, 0, 10)
    b, _ = make_pair(pkg, O, 1024, 3072, 0, 10)
    tgt, _ = target_audio(O, 0, a.N)
    for e in (a, b):
        e.set_target_audio(tgt)
        e.init_population(0)
    a.execute_generations(6)
    for _ in range(6):
        b.execute_generation()
    for x, y in zip(a.read_population(), b.read_population()):
        assert np.array_equal(x, y, equal_nan=True)
    a.close(); b.close()
