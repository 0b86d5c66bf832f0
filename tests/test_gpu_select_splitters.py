"""The one-launch selection (k_sel_splitters, plan SPLITTERS / AUTO): the rows of the two-launch selection bit for bit,
whatever the splitter slot holds."""
import time

import numpy as np
import pytest

from test_gpu_parity import PMAX, SELECT_CASES, fitness_pattern, make_pair, target_audio
from test_select_splitters_model import make_keys, rank_step

pytestmark = pytest.mark.gpu

SMALL_CASES = [c for c in SELECT_CASES if c[0] + c[1] <= 65536]


def select_and_check(pkg, O, es, parents, f, v, s):
    """test_select_places_exactly_the_rows_recombination_reads' protocol on a context whose slot is prepared"""
    P, D = es.P, es.D
    S = max(parents, max(1, parents // 32) * 32)
    sentinel_v = np.full((P, D), -7.0, np.float32)
    es.set_sort_mode(pkg.capi.SORT_TOP_ONLY)
    es.write_population(sentinel_v, sentinel_v, np.full(P, -7.0, np.float32))  # the half the selection writes into
    es.rotate()
    es.write_population(v, s, f)
    es.select(); es.rotate()
    gv, gs, gf = es.read_population()
    perm = O.sort_perm(f)
    assert np.array_equal(gf[:S], f[perm][:S], equal_nan=True)
    assert np.array_equal(gv[:S], v[perm][:S]) and np.array_equal(gs[:S], s[perm][:S])
    if 1024 < P <= 131072 and 2 * S <= P:
        assert np.all(gf[S:] == -7.0) and np.all(gv[S:] == -7.0) and np.all(gs[S:] == -7.0), "rows beyond S were written"
    es.set_sort_mode(pkg.capi.SORT_LAZY_TAIL)  # the rest of the order on demand, from the untouched unsorted half
    gv, gs, gf = es.read_population()
    assert np.array_equal(gf, f[perm], equal_nan=True) and np.array_equal(gv, v[perm]) and np.array_equal(gs, s[perm])
    ov, os_, of = es.read_population(other=True)
    assert np.array_equal(ov, v) and np.array_equal(os_, s) and np.array_equal(of, f, equal_nan=True)


def prime(pkg, es, f):
    """one selection of fitness f: leaves ITS splitters in the slot the next selection reads"""
    es.set_sort_mode(pkg.capi.SORT_TOP_ONLY)
    z = np.zeros((es.P, es.D), np.float32)
    es.write_population(z, z, f)
    es.select(); es.rotate()


@pytest.mark.parametrize("parents,offspring,kind,pattern", SMALL_CASES)
def test_splitters_plan_fresh_and_stale(pkg, O, parents, offspring, kind, pattern):
    """after a selection of the same pattern (fresh splitters) and after one of a different pattern (stale ones)"""
    es, _ = make_pair(pkg, O, parents, offspring, kind, 9)
    es.set_select_plan(pkg.capi.SELECT_SPLITTERS)
    rng = np.random.default_rng(parents + len(pattern))
    P, D = es.P, es.D
    f = fitness_pattern(pattern, P, rng)
    v = rng.random((P, D), dtype=np.float32)
    s = rng.random((P, D), dtype=np.float32)
    prime(pkg, es, fitness_pattern(pattern, P, rng))
    select_and_check(pkg, O, es, parents, f, v, s)
    prime(pkg, es, fitness_pattern("tile_skew" if pattern != "tile_skew" else "descending", P, rng))
    select_and_check(pkg, O, es, parents, f, v, s)
    es.close()


def test_splitters_plan_denormals_and_bound_ties(pkg, O):
    """fitness values down in the denormals (a converged run gets there), signed zeros, and splitters that ARE keys of the
    population (its own, one selection earlier): the stream's float compares must order them as the key bits do"""
    parents, offspring = 16384, 49152
    es, _ = make_pair(pkg, O, parents, offspring, 0, 9)
    es.set_select_plan(pkg.capi.SELECT_SPLITTERS)
    rng = np.random.default_rng(11)
    P, D = es.P, es.D
    f = (rng.random(P) * 1e-38).astype(np.float32)                 # half of them below the smallest normal number
    f[rng.choice(P, P // 8, replace=False)] = np.float32(1e-45)    # the smallest denormal, many times
    f[rng.choice(P, P // 16, replace=False)] = 0.0
    f[rng.choice(P, P // 16, replace=False)] = -0.0
    f[rng.choice(P, 100, replace=False)] = -np.float32(3e-42)
    v = rng.random((P, D), dtype=np.float32)
    s = rng.random((P, D), dtype=np.float32)
    prime(pkg, es, f)
    select_and_check(pkg, O, es, parents, f, v, s)
    prime(pkg, es, np.roll(f, 12345))
    select_and_check(pkg, O, es, parents, f, v, s)
    es.close()


def degenerate(name, B, f, rng):
    keys = np.sort(make_keys(f))
    if name == "zero":
        return np.zeros(B, np.uint64)
    if name == "ones":
        return np.full(B, 0xFFFFFFFFFFFFFFFF, np.uint64)
    if name == "constant":      # one bucket below the median key, one above: each more than a third of the keys
        return np.full(B, keys[len(keys) // 2], np.uint64)
    if name == "descending":
        return keys[(np.arange(B) * (len(keys) // B))[::-1]].copy()
    if name == "one_huge":      # fine splitters over the best 1 %, then one workgroup owns the rest
        return keys[np.arange(B) * max(1, len(keys) // (100 * B))].copy()
    if name == "nan_region":
        return (np.uint64(0xFFFFFFFD) << np.uint64(32)) | rng.integers(0, len(f), B).astype(np.uint64)
    return rng.integers(0, 1 << 63, B, dtype=np.uint64) * np.uint64(2)  # garbage


@pytest.mark.parametrize("parents,offspring,kind,pattern", SMALL_CASES)
def test_splitters_plan_degenerate_slots(pkg, O, parents, offspring, kind, pattern):
    """hand-written slots: the slow path (one workgroup owns more than half of the keys), empty buckets, bounds above
    every number"""
    es, _ = make_pair(pkg, O, parents, offspring, kind, 9)
    es.set_select_plan(pkg.capi.SELECT_SPLITTERS)
    rng = np.random.default_rng(parents + 7 * len(pattern))
    P, D = es.P, es.D
    f = fitness_pattern(pattern, P, rng)
    v = rng.random((P, D), dtype=np.float32)
    s = rng.random((P, D), dtype=np.float32)
    B = es.select_splitter_count()
    for name in ("zero", "ones", "constant", "descending", "one_huge", "nan_region", "garbage"):
        es.write_select_splitters(degenerate(name, B, f, rng))
        select_and_check(pkg, O, es, parents, f, v, s)
    es.close()


def test_slot_after_a_selection_holds_the_rank_step_keys(pkg, O):
    es, _ = make_pair(pkg, O, 16384, 49152, 0, 9)
    es.set_select_plan(pkg.capi.SELECT_SPLITTERS)
    rng = np.random.default_rng(3)
    f = fitness_pattern("random", es.P, rng)
    prime(pkg, es, f)
    B = es.select_splitter_count()
    step = rank_step(16384, B)
    got = es.read_select_splitters()
    assert np.array_equal(got[1:], np.sort(make_keys(f))[np.arange(1, B) * step]) and got[0] == 0
    es.close()


def test_slow_path_worst_case_finishes(pkg, O):
    """all-zero splitters at P = 65536: the last workgroup owns every key and orders them alone in global memory.
    The bound is not a speed target: 136 network steps of 32 768 compare-exchanges by 1024 threads, each step a round trip
    to L2 behind a workgroup barrier (some 10 us), come to 1-2 ms, and half a second is what any test here can wait for
    a single launch; measured 2.2 ms on an MI355X."""
    es, _ = make_pair(pkg, O, 16384, 49152, 0, 9)
    es.set_select_plan(pkg.capi.SELECT_SPLITTERS)
    rng = np.random.default_rng(5)
    f = fitness_pattern("random", es.P, rng)
    z = np.zeros((es.P, es.D), np.float32)
    es.set_sort_mode(pkg.capi.SORT_TOP_ONLY)
    B = es.select_splitter_count()
    times = []
    for _ in range(3):
        es.write_population(z, z, f)
        es.write_select_splitters(np.zeros(B, np.uint64))
        es.synchronize()
        t = time.perf_counter()
        es.select()
        es.synchronize()
        times.append(time.perf_counter() - t)
        es.rotate()
    print(f"slow path, one workgroup orders 65536 keys: {min(times) * 1e3:.2f} ms (best of 3)")
    gf = es.read_fitness()
    assert np.array_equal(gf[:16384], f[O.sort_perm(f)][:16384])
    assert min(times) < 0.5, "the slow path must stay far inside any test's time limit"
    es.close()


def run_pair(pkg, O, parents, offspring, gens, every, reinit_at=None):
    a, _ = make_pair(pkg, O, parents, offspring, 0, 10)
    b, _ = make_pair(pkg, O, parents, offspring, 0, 10)
    b.set_select_plan(pkg.capi.SELECT_TILES)
    tgt, _ = target_audio(O, 0, a.N)
    for es in (a, b):
        es.set_target_audio(tgt)
        es.init_population(0)
    for g in range(0, gens, every):
        if reinit_at is not None and g == reinit_at:
            for es in (a, b):
                es.init_population(1)
        for es in (a, b):
            es.execute_generations(every)
        for x, y in zip(a.read_population(), b.read_population()):
            assert np.array_equal(x, y, equal_nan=True), f"generation {g + every}"
    a.close(); b.close()


def test_fused_loop_auto_equals_tiles_200_generations(pkg, O):
    """configs[2]'s population: AUTO (splitters from the second generation on) against TILES, every 25 generations"""
    run_pair(pkg, O, 16384, 49152, 200, 25)


def test_fused_loop_reinitialised_in_the_middle(pkg, O):
    """a new population under the old population's splitters: the first generation falls back, then the run goes on"""
    run_pair(pkg, O, 16384, 49152, 60, 10, reinit_at=30)
    run_pair(pkg, O, 2048, 6144, 24, 3, reinit_at=12)


def test_fused_loop_top_only_mode(pkg, O):
    """SORT_TOP_ONLY under AUTO: the selected rows equal the lazy-tail run's"""
    a, _ = make_pair(pkg, O, 4096, 12288, 0, 10)
    b, _ = make_pair(pkg, O, 4096, 12288, 0, 10)
    a.set_sort_mode(pkg.capi.SORT_TOP_ONLY)
    b.set_select_plan(pkg.capi.SELECT_TILES)
    tgt, _ = target_audio(O, 0, a.N)
    for es in (a, b):
        es.set_target_audio(tgt)
        es.init_population(0)
        es.execute_generations(7)
    for x, y in zip(a.read_population(), b.read_population()):
        assert np.array_equal(x[:4096], y[:4096])
    a.close(); b.close()


@pytest.mark.parametrize("parents,offspring", [(16384, 49152), (2048, 6144)])
def test_two_islands_exchange_every_generation(pkg, O, parents, offspring):
    """the island exchange carried inside the selection kernel (immigrant rows, elite sink): a group under AUTO against
    the same group under TILES"""
    target = O.synth(0, [1450 / 3520, 3 / 8, 200 / 3520, 1.0], [0.0] * 4, PMAX[0], 1024)
    groups = []
    for plan in (pkg.capi.SELECT_AUTO, pkg.capi.SELECT_TILES):
        g = pkg.HipGroup([0, 0], 16, parents, offspring, pkg.capi.SYNTH_2OP, 10, None, PMAX[0], seed=0x5EED0001,
                         migration_interval=1, overlap=True)
        for r in range(2):
            g.island(r).set_select_plan(plan)
        g.set_target_audio(target)
        g.init_population(0)
        groups.append(g)
    for chunk in range(4):
        for g in groups:
            g.execute_generations(25)
            g.synchronize()
        for r in range(2):
            for x, y in zip(groups[0].island(r).read_population(), groups[1].island(r).read_population()):
                assert np.array_equal(x, y, equal_nan=True), f"island {r} after {25 * (chunk + 1)} generations"
    for g in groups:
        g.close()
