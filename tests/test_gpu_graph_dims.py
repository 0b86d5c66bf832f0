"""Everything but synthesis at the widths only the operator-graph voice has: D = 10, 14 and 16 (graphs stacks5, seven and
dense8 of tests/_graph_voice_model.py).  The fixed voices stop at D = 12, so these are the first rows of 2 D + 1 = 21, 29
and 33 floats that initialisation, variation, the sorts, both selection plans, the run record, batch and queue see:
Philox block 3 of k_init_population, g (b + 1) up to g = 15 in recombine_source, the mutation constants of 1/D and
sqrt(1/D), the last column round of k_sel_rank_scatter (column 32 is the fitness only at D = 16), k_track's threads / d
lanes and its row copy, and the queue's result rows with all sixteen entries live.

The stages are fed by write_population, so each is judged from inputs written here against the references the fixed
voices are judged by: tests/_variation_model.py (steps within its STEP_RTOL against fp64, values bit for bit), the stable
order by (fitness, index), a twin trajectory for the run record, sequential tracked contexts for batch and queue.
Each case that judges steps prints a line `VARIATION {...}`; profiles/r23_graph_dims.json collects them."""
import numpy as np
import pytest

import _variation_model as vm
from _graph_voice_model import GRAPHS
from _survivors_model import targets
from test_gpu_parity import fitness_pattern, sort_case
from test_gpu_run_record import check_best_ever, check_history
from test_gpu_select_splitters import prime, select_and_check
from test_gpu_variation import init_words, judge, same_bits, staged_generation

pytestmark = pytest.mark.gpu

BY_DIMS = {10: "stacks5", 14: "seven", 16: "dense8"}
WIDTHS = sorted(BY_DIMS)
M32 = 0xFFFFFFFF


def pmax_of(name):
    """frequencies up to 3520 Hz, modulation indices up to 8, carrier levels up to 1"""
    ops, _, carriers = GRAPHS[name]
    out = []
    for j in range(ops):
        out += [3520.0, 1.0 if carriers >> j & 1 else 8.0]
    return out


def graph_context(pkg, name, parents, offspring, block=32, log2n=vm.N_LOG2, slots=0, target=True, survivors=0, generation=None):
    """a HipES of graph `name` - or, with slots, a tracked HipBatch of that many slots"""
    kw = dict(synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=log2n, param_max=pmax_of(name), seed=vm.SEED, workgroup_size=block,
              graph=pkg.capi.make_voice_graph(*GRAPHS[name]))
    if slots:
        b = pkg.HipBatch(slots, parents, offspring, **kw)
        b.track()
        b.set_survivors(survivors)
        return b
    es = pkg.HipES(parents, offspring, **kw)
    assert es.D == 2 * GRAPHS[name][0]
    if target:
        es.set_target_audio(targets(1, 1 << log2n)[0])
    if survivors:
        es.set_survivors(survivors)
    if generation is not None:
        es.generation = generation
    return es


def random_rows(p, d, seed):
    rng = np.random.default_rng(seed)
    return rng, rng.random((p, d), dtype=np.float32), rng.random((p, d), dtype=np.float32)


# ---- 1. initialisation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDTHS)
def test_init_population(pkg, O, d):
    """genes 12 to 15 take their word from Philox block 3"""
    p = 96
    es = graph_context(pkg, BY_DIMS[d], 32, 64, target=False)
    for chunk in (0, vm.EDGE_CHUNK):
        es.init_population(chunk)
        gv, gs, _ = es.read_population()
        mv, ms = vm.init(init_words(O, p, d, 0, chunk))
        assert same_bits(gv, mv) and same_bits(gs, ms), f"init_population({chunk:#x})"
    es.close()


# ---- 2. recombination -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parents,block", [(80, 24), (96, 32), (80, 384)])
@pytest.mark.parametrize("d", WIDTHS)
def test_recombine(pkg, d, parents, block):
    """3 parent blocks of 24 (divide / modulo), 3 of 32 (shifts and masks), and one block that is the population"""
    p = 384
    _, v, s = random_rows(p, d, p * 31 + block + d)
    es = graph_context(pkg, BY_DIMS[d], parents, p - parents, block=block, target=False)
    es.write_population(v, s, np.zeros(p, np.float32))
    es.recombine()
    gv, gs, _ = es.read_population()
    ov, os_, _ = es.read_population(other=True)
    es.close()
    mv, ms = vm.recombine(v, s, parents, block)
    assert same_bits(gv, mv), int(np.count_nonzero(gv != mv))
    assert same_bits(gs, ms), int(np.count_nonzero(gs != ms))
    assert same_bits(ov, v) and same_bits(os_, s), "recombine wrote to its source half"


# ---- 3. mutation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDTHS)
def test_mutate_step_and_value_edges(pkg, O, d):
    """stage calls only: these genes are never synthesised"""
    p = vm.EDGE_ROWS
    v, s = vm.edge_population(d)
    es = graph_context(pkg, BY_DIMS[d], 1024, p - 1024, target=False)
    for gen in (vm.SITE_GENERATION, M32):
        es.write_population(v, s, np.zeros(p, np.float32))
        es.generation = gen
        es.mutate()
        gv, gs, _ = es.read_population()
        mv, ms = vm.mutate(v, s, O.mutate_words(p, d, vm.SEED, 0, gen), d)
        judge(gv, gs, mv, ms, part="edges", site="k_mutate", P=p, D=d, generation=gen)
        zero, inf, nan = ms == 0.0, np.isinf(ms), np.isnan(ms)
        assert zero.any() and inf.any() and nan.any()
        assert np.all(gs[zero] == 0.0) and np.all(gs[inf] == ms[inf].astype(np.float32)) and np.array_equal(np.isnan(gs), nan)
    es.close()


# ---- 4. one generation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", vm.SITE_SURVIVORS)
@pytest.mark.parametrize("d", WIDTHS)
def test_one_generation(pkg, O, d, k):
    """test_gpu_variation.site_case for a graph context: the staged pre-sort population equals the model, one fused
    generation equals the staged one bit for bit, and the variation launch is there, since k_synth_graph makes no individuals"""
    name, p = BY_DIMS[d], 768
    parents, block, gen = vm.SITE_PARENTS, vm.SITE_BLOCK, vm.SITE_GENERATION
    v, s = vm.site_population(p, d, p + d)
    zero = np.zeros(p, np.float32)
    a = graph_context(pkg, name, parents, p - parents, block=block, survivors=k, generation=gen)
    b = graph_context(pkg, name, parents, p - parents, block=block, survivors=k, generation=gen)
    for e in (a, b):
        e.write_population(v, s, zero)
    pv, ps = staged_generation(b)
    a.timing_enable(True)
    a.execute_generations(1)
    _, launches = a.stage_time_ms(pkg.capi.STAGE_FUSED_VARIATION)
    fused, staged = a.read_population(), b.read_population()
    a.close(); b.close()
    mv, ms = vm.generation(v, s, parents, block, O.mutate_words(p, d, vm.SEED, 0, gen), k)
    judge(pv, ps, mv, ms, part="site", site=f"k_recombine_mutate<graph {name}>", P=p, D=d, block=block, parents=parents, survivors=k)
    if k:
        assert same_bits(pv[:k], v[:k]) and same_bits(ps[:k], s[:k]), "a survivor changed"
    assert launches == 1, launches
    for x, y, label in zip(fused, staged, ("values", "steps", "fitness")):
        assert same_bits(x, y), (label, int(np.count_nonzero(x != y)))
    assert np.all(np.isfinite(fused[2]))


# ---- 5. sorting -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,parents,p,block", [
    (16, 40, 1000, 40),         # one launch, one workgroup, 24 padding keys
    (16, 50, 2050, 50),         # 1024-key tiles and one rank level, just above two tiles
    (16, 32768, 131072, 32),    # tiles merged into runs and a rank level over the runs
    (10, 40, 1000, 40), (10, 50, 2050, 50)])
def test_sort_matches_the_stable_order(pkg, O, d, parents, p, block):
    """rows of 2 D + 1 floats through k_sort_small and k_sort_rank_scatter: ties, NaN, inf and signed zeros in the fitness"""
    es = graph_context(pkg, BY_DIMS[d], parents, p - parents, block=block, target=False)
    es.set_sort_mode(pkg.capi.SORT_FULL)
    rng, v, s = random_rows(p, d, p + d)
    f = sort_case(p, rng)
    f[::97] = f[5]  # many duplicates, across tiles where there are tiles
    es.write_population(v, s, f)
    es.sort(); es.rotate()
    gv, gs, gf = es.read_population()
    es.close()
    perm = O.sort_perm(f)
    assert np.array_equal(gf, f[perm], equal_nan=True)
    assert np.array_equal(gv, v[perm]) and np.array_equal(gs, s[perm])


# ---- 6. selection, both plans ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["few_values", "constant"])
@pytest.mark.parametrize("plan", [1, 2], ids=["tiles", "splitters"])
@pytest.mark.parametrize("parents,p", [(1024, 4096), (4096, 16384)], ids=["staged-whole", "not-staged-whole"])
@pytest.mark.parametrize("d", WIDTHS)
def test_select_places_exactly_the_rows_recombination_reads(pkg, O, d, parents, p, plan, pattern):
    """the protocol of tests/test_gpu_parity.py and tests/test_gpu_select_splitters.py (sentinel rows beyond S, the lazy
    tail, the other half intact) on rows of 21, 29 and 33 floats, under massive ties and under one value throughout"""
    es = graph_context(pkg, BY_DIMS[d], parents, p - parents, log2n=9, target=False)
    es.set_select_plan(plan)
    rng, v, s = random_rows(p, d, parents + len(pattern) + d)
    f = fitness_pattern(pattern, p, rng)
    if plan == pkg.capi.SELECT_SPLITTERS:
        prime(pkg, es, fitness_pattern(pattern, p, rng))  # leaves splitters of the same kind of fitness in the slot
    select_and_check(pkg, O, es, parents, f, v, s)
    es.close()


# ---- 7. list mode ---------------------------------------------------------------------------------------------------------------
def test_three_generations_under_lists_equal_three_under_tiles(pkg):
    """dense8 at N = 1024 and P = 4096 >= 12 x 256: the wide spectral kernel files the keys (select_lists_apply) and from
    the second generation AUTO selects from the lists; plan TILES never does"""
    parents, p = 1024, 4096
    a = graph_context(pkg, "dense8", parents, p - parents, log2n=10)
    b = graph_context(pkg, "dense8", parents, p - parents, log2n=10)
    b.set_select_plan(pkg.capi.SELECT_TILES)
    for es in (a, b):
        es.init_population(0)
        es.execute_generations(3)
    got, want = a.read_population(), b.read_population()
    a.close(); b.close()
    for x, y, label in zip(got, want, ("values", "steps", "fitness")):
        assert same_bits(x, y), label
    assert np.all(np.isfinite(want[2])) and np.all(np.diff(want[2]) >= 0)


# ---- 8. run record --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,parents,offspring,gens", [
    (10, 32, 32, 8), (10, 1024, 3072, 3),    # parents x D <= 8192: k_track with 256 threads, 25 lanes of 10; above: 1024, 102 lanes
    (14, 96, 160, 8), (14, 1024, 3072, 3),   # 18 lanes of 14; 73
    (16, 16, 16, 8), (16, 1024, 3072, 3)])   # 16 lanes of 16; 64
def test_history_and_best_ever_against_a_twin(pkg, d, parents, offspring, gens):
    name = BY_DIMS[d]
    twin = graph_context(pkg, name, parents, offspring)
    twin.init_population(0)
    traj = []
    for _ in range(gens):
        twin.execute_generations(1)
        traj.append(twin.read_population())
    twin.close()
    es = graph_context(pkg, name, parents, offspring)
    es.init_population(0)
    es.track(history_every=1, capacity=gens)
    es.execute_generations(gens)
    hist, taken = es.history(with_taken=True)
    assert taken == gens
    check_history(hist, traj, parents, d, range(1, gens + 1))
    assert np.all(hist["mean_step"][:, :d] > 0) and np.all(hist["mean_step"][:, d:] == 0)
    check_best_ever(es, traj)
    for x, y in zip(es.read_population(), traj[-1]):
        assert same_bits(x, y), "tracking changed the population"
    es.close()


# ---- 9. batch and queue ---------------------------------------------------------------------------------------------------------
SMALL = dict(parents=32, offspring=32)
STALL = dict(target=None, stall=20, check_every=10)
RESULT_FLOATS = ("best_ever_fitness", "last_fitness", "best_ever_values", "best_ever_steps", "last_values")


def test_three_chunks_in_a_batch_equal_three_contexts(pkg):
    name, gens = "dense8", 30
    tg = targets(3, 1 << vm.N_LOG2)
    b = graph_context(pkg, name, **SMALL, slots=3)
    b.set_target_audio(tg)
    b.init_population(0)
    b.execute_generations(gens)
    bv, bs, bf, bg = b.best_ever()
    es = graph_context(pkg, name, **SMALL)
    es.track()
    for c in range(3):
        es.set_target_audio(tg[c])
        es.init_population(c)
        es.execute_generations(gens)
        for what, x, y in zip(("values", "steps", "fitness"), b.read_population(c), es.read_population()):
            assert same_bits(x, y), (c, what)
        v, s, f, g = es.best_ever()
        assert same_bits(bv[c], v) and same_bits(bs[c], s) and same_bits(bf[c], f) and bg[c] == g, c
    es.close()
    b.close()


def sequential_reference(pkg, es, tg, max_g, rule, rows, segment):
    """the sequence include/sots_hip.h gives as the definition of the queue with carried rows, on one tracked context: a
    chunk that is not the first of its segment starts from init_population with rows 0..rows-1 written over by the state
    its predecessor left - row 0 the best-ever record, rows 1.. those of the sorted half"""
    d = es.D
    out = np.zeros(len(tg), pkg.capi.CHUNK_RESULT_DTYPE)
    for k in range(len(tg)):
        successor = rows > 0 and k % segment != 0
        if successor:
            pv, ps, _ = es.read_population()
            bv, bs, _, _ = es.best_ever()
        es.set_target_audio(tg[k])
        es.init_population(k)
        if successor:
            v, s, _ = es.read_population()
            v[:rows], s[:rows] = pv[:rows], ps[:rows]
            v[0], s[0] = bv, bs
            es.write_population(v, s, None)
        run = es.execute_until(max_g, **rule)
        v, s, f, g = es.best_ever()
        pop = es.read_population()
        r = out[k]
        r["generations_run"], r["best_ever_generation"], r["best_ever_fitness"], r["last_fitness"] = run, g, f, pop[2][0]
        r["best_ever_values"][:d], r["best_ever_steps"][:d], r["last_values"][:d] = v, s, pop[0][0]
    return out


@pytest.mark.parametrize("rows", [0, 2], ids=["plain", "carry2"])
@pytest.mark.parametrize("d", [10, 16])
def test_three_chunks_through_a_two_slot_queue_equal_three_contexts(pkg, d, rows):
    """a stall rule; with carried rows, segments of two chunks (chunk 1 starts from what chunk 0 left, chunk 2 afresh).
    The result rows hold sixteen entries: all of them live at D = 16, entries 10.. zero at D = 10"""
    name, max_g, segment = BY_DIMS[d], 100, 2
    tg = targets(3, 1 << vm.N_LOG2)
    es = graph_context(pkg, name, **SMALL, survivors=1)
    es.track()
    want = sequential_reference(pkg, es, tg, max_g, STALL, rows, segment)
    es.close()
    b = graph_context(pkg, name, **SMALL, slots=2, survivors=1)
    b.queue_set_carry(rows, segment)
    b.queue_targets_audio(tg)
    got, stats = b.queue_run(0, max_g, **STALL)
    b.close()
    assert len(got) == 3
    for k in range(3):
        for field in ("generations_run", "best_ever_generation"):
            assert got[k][field] == want[k][field], (k, field, got[k][field], want[k][field])
        for field in RESULT_FLOATS:
            assert same_bits(got[k][field], want[k][field]), (k, field, got[k][field], want[k][field])
        for field in ("best_ever_values", "best_ever_steps", "last_values"):
            assert np.all(got[k][field][:d] != 0) and np.all(got[k][field].view(np.uint32)[d:] == 0), (k, field)
    runs = want["generations_run"]
    sums = [int(runs[0]) + int(runs[1]), int(runs[2])] if rows else [int(r) for r in runs]
    assert stats["slots"] == 2 and stats["chunk_generations"] == int(runs.sum())
    assert stats["global_generations"] == pkg.HipBatch.queue_makespan(np.asarray(sums, np.uint32), 2)
