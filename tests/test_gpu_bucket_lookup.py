"""The key-filing hook's bucket lookup on the GPU (bkt_visit), at the smallest population at which the twelve-wavefront
spectral kernel files keys and the one-launch selection applies: P = 4096 = 1024 + 3072, 2-op, N = 1024.  The slots put
every bound - every lane's share of the bounds and the open-bucket edge - among the S = 1024 rows that are compared bit
for bit with the stable sort."""
import numpy as np
import pytest

from test_gpu_parity import make_pair, target_audio
from test_gpu_select_lists import make_es, select_and_check
from test_select_splitters_model import make_keys

pytestmark = pytest.mark.gpu

PARENTS, OFFSPRING = 1024, 3072
P = PARENTS + OFFSPRING


def fitness(pattern, rng):
    if pattern == "distinct":
        return rng.permutation(P).astype(np.float32) / np.float32(P)
    if pattern == "runs":       # runs of 6 equal values over bounds 4 ranks apart: every run holds a bound or two
        return (rng.permutation(P) // 6).astype(np.float32)
    return np.full(P, 0.25, np.float32)     # one value for all rows: the row index decides


@pytest.fixture(scope="module")
def es(pkg, O):
    e, _ = make_pair(pkg, O, PARENTS, OFFSPRING, 0, 10)
    e.set_select_plan(pkg.capi.SELECT_SPLITTERS)
    yield e
    e.close()


@pytest.mark.parametrize("pattern", ["distinct", "runs", "tie"])
def test_stage_path_with_every_bound_among_the_compared_rows(pkg, O, es, pattern):
    rng = np.random.default_rng(19 + len(pattern))
    f = fitness(pattern, rng)
    v = rng.random((P, es.D), dtype=np.float32)
    s = rng.random((P, es.D), dtype=np.float32)
    B = es.select_splitter_count()
    k = np.sort(make_keys(f))
    every = k[np.arange(B) * ((PARENTS - 1) // (B - 1))].copy()    # all B - 1 bounds are keys at ranks below S
    half = k[np.arange(B) * max(1, PARENTS // (2 * B))].copy()
    half[-1] = k[PARENTS // 2]                                      # the last bound at rank S / 2: half the selected rows are open-bucket rows
    wide = half.copy()
    wide[-1] = k[PARENTS // 2 - 1] | np.uint64(0x80000000)         # ... and a last bound that is no key: its index word has the top bit set
    ones = np.full(B, 0xFFFFFFFFFFFFFFFF, np.uint64)
    for slot in (every, half, wide, ones):
        select_and_check(pkg, O, es, PARENTS, f, v, s, slot)


def test_fused_loop_lists_equal_tiles_40_generations(pkg, O):
    """generation 0 takes the two-launch path and seeds the slot, as in the product; from then on the spectral kernel
    files the keys (AUTO) - the populations are those of plan TILES byte for byte"""
    pair = [make_es(pkg, O, PARENTS, OFFSPRING), make_es(pkg, O, PARENTS, OFFSPRING, plan=pkg.capi.SELECT_TILES)]
    tgt, _ = target_audio(O, 0, pair[0].N)
    for e in pair:
        e.set_target_audio(tgt)
        e.init_population(0)
    for g in range(0, 40, 10):
        got = []
        for e in pair:
            e.execute_generations(10)
            got.append(e.read_population())
        for x, y in zip(*got):
            assert np.array_equal(x, y, equal_nan=True), f"generation {g + 10}"
    for e in pair:
        e.close()
