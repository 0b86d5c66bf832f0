"""Variation on the GPU at the sizes the rest of the suite leaves out: recombination blocks and parent-block counts that are
no powers of two (recombine_source's divide / modulo path) at every site of make_gene, selection under such blocks, steps
and values at the edges of fp32, and Philox counters that wrap.

The reference is tests/_variation_model.py: recombination as a scatter in 64-bit integers, the value half of mutation in
np.float32 in the kernel's written order (bit for bit), the new step in fp64 (the device within
|s_dev - s_64| <= 2e-6 |s_64| + 2^-149, vm.step_ratio).  tests/test_variation_cpu.py shows, without a GPU, that the model is
the oracle's rule, that a wrong recombination is caught by the geometries below, and that every population written here
takes both coins and both sides of the reflect branch.

Each case that judges steps prints a line `VARIATION {...}` with its worst |ds| / bound; profiles/r21_variation.json
collects them.  The case lists (with the dispatcher rule that selects each site on 256 CUs) are in the model's module."""
import json

import numpy as np
import pytest

import _variation_model as vm
from _survivors_model import PMAX, targets

pytestmark = pytest.mark.gpu

DIMS = {0: 4, 1: 6, 2: 12, 3: 8}
N = 1 << vm.N_LOG2
M32 = 0xFFFFFFFF
SITE_IDS = [s[0].replace("<", "-").replace(">", "").replace(",", "-").replace(" ", "-") for s in vm.SITES]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def make(pkg, kind, parents, offspring, block, gid_base=0, k=0, generation=None):
    es = pkg.HipES(parents, offspring, synth_kind=kind, audio_log2=vm.N_LOG2, param_max=PMAX[kind], seed=vm.SEED, workgroup_size=block,
                   gid_base=gid_base)
    es.set_target_audio(targets(1, N)[0])
    if k:
        es.set_survivors(k)
    if generation is not None:
        es.generation = generation
    return es


def judge(got_v, got_s, want_v, want_s64, **case):
    """values bit for bit (a NaN for a NaN), steps within the bound; prints the worst |ds| / bound"""
    ratio = vm.step_ratio(got_s, want_s64)
    worst = int(np.argmax(ratio))
    print("VARIATION " + json.dumps({**case, "worst_ds_over_bound": float(f"{ratio.flat[worst]:.4g}")}))
    assert np.array_equal(np.isnan(got_v), np.isnan(want_v)), case
    assert vm.same_values(got_v, want_v), (case, int(np.count_nonzero(bits(got_v) != bits(want_v))))
    assert np.all(ratio <= 1.0), (case, worst, float(np.asarray(got_s).flat[worst]), float(want_s64.flat[worst]), float(ratio.flat[worst]))


def staged_generation(es):
    """one stage-separated generation; returns the pre-sort population (values, steps)"""
    es.recombine(); es.mutate()
    v, s, _ = es.read_population()
    es.synthesise(); es.window(); es.fft(); es.fitness(); es.sort(); es.rotate()
    return v, s


# ---- (a) geometry, stage kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,parents,offspring,block", vm.GEOMETRIES)
def test_recombine_geometry(pkg, kind, parents, offspring, block):
    p, d = parents + offspring, DIMS[kind]
    rng = np.random.default_rng(p * 31 + block)
    v, s = rng.random((p, d), dtype=np.float32), rng.random((p, d), dtype=np.float32)
    es = make(pkg, kind, parents, offspring, block)
    es.write_population(v, s, np.zeros(p, np.float32))
    es.recombine()
    gv, gs, _ = es.read_population()
    ov, os_, _ = es.read_population(other=True)
    es.close()
    mv, ms = vm.recombine(v, s, parents, block)
    assert same_bits(gv, mv), int(np.count_nonzero(bits(gv) != bits(mv)))
    assert same_bits(gs, ms), int(np.count_nonzero(bits(gs) != bits(ms)))
    assert same_bits(ov, v) and same_bits(os_, s), "recombine wrote to its source half"


# ---- (b) geometry, every site ---------------------------------------------------------------------------------------------------
def site_case(pkg, O, name, kind, p, in_synth, k, v, s, what):
    """staged pre-sort population == model; one fused generation == the staged one, bit for bit; the variation launch is
    there exactly where the dispatcher rule says no synthesis kernel makes the individuals"""
    d = DIMS[kind]
    parents, block, gen = vm.SITE_PARENTS, vm.SITE_BLOCK, vm.SITE_GENERATION
    zero = np.zeros(p, np.float32)
    a = make(pkg, kind, parents, p - parents, block, k=k, generation=gen)
    b = make(pkg, kind, parents, p - parents, block, k=k, generation=gen)
    for e in (a, b):
        e.write_population(v, s, zero)
    pv, ps = staged_generation(b)
    a.timing_enable(True)
    a.execute_generations(1)
    _, launches = a.stage_time_ms(pkg.capi.STAGE_FUSED_VARIATION)
    fused, staged = a.read_population(), b.read_population()
    a.close(); b.close()
    mv, ms = vm.generation(v, s, parents, block, O.mutate_words(p, d, vm.SEED, 0, gen), k)
    judge(pv, ps, mv, ms, part=what, site=name, P=p, D=d, block=block, parents=parents, survivors=k)
    if k:
        assert same_bits(pv[:k], v[:k]) and same_bits(ps[:k], s[:k]), "a survivor changed"
    assert launches == (0 if in_synth else 1), (name, launches)
    for x, y, label in zip(fused, staged, ("values", "steps", "fitness")):
        assert same_bits(x, y), (name, label, int(np.count_nonzero(bits(x) != bits(y))))
    assert np.all(np.isfinite(fused[2])), name


@pytest.mark.parametrize("k", vm.SITE_SURVIVORS)
@pytest.mark.parametrize("name,kind,p,in_synth", vm.SITES, ids=SITE_IDS)
def test_site(pkg, O, name, kind, p, in_synth, k):
    v, s = vm.site_population(p, DIMS[kind], p + kind)
    site_case(pkg, O, name, kind, p, in_synth, k, v, s, "site")


@pytest.mark.parametrize("kind", [0, 2])
@pytest.mark.parametrize("k", vm.SITE_SURVIVORS)
def test_batch_chunks_equal_contexts(pkg, kind, k):
    """k_recombine_mutate_seg (HipBatch.execute_generations): three chunks, three generations, block 24, 3 parent blocks"""
    parents, p, block, chunks = vm.SITE_PARENTS, 768, vm.SITE_BLOCK, 3
    tg = targets(chunks, N)
    kw = dict(synth_kind=kind, audio_log2=vm.N_LOG2, param_max=PMAX[kind], seed=vm.SEED, workgroup_size=block)
    b = pkg.HipBatch(chunks, parents, p - parents, **kw)
    b.set_survivors(k)
    b.set_target_audio(tg)
    b.init_population(5)
    b.execute_generations(3)
    es = pkg.HipES(parents, p - parents, **kw)
    es.set_survivors(k)
    for c in range(chunks):
        es.set_target_audio(tg[c])
        es.init_population(5 + c)
        es.execute_generations(3)
        for x, y in zip(b.read_population(c), es.read_population()):
            assert same_bits(x, y), f"chunk {c}"
    b.close(); es.close()


@pytest.mark.parametrize("k", vm.SITE_SURVIVORS)
def test_queue_chunks_equal_contexts(pkg, k):
    """k_recombine_mutate_queue (queue_run with no stop rule): five chunks through two slots, four generations each"""
    kind, parents, p, block, chunks, keep, gens = 1, vm.SITE_PARENTS, 768, vm.SITE_BLOCK, 5, 3, 4
    d = DIMS[kind]
    tg = targets(chunks, N)
    kw = dict(synth_kind=kind, audio_log2=vm.N_LOG2, param_max=PMAX[kind], seed=vm.SEED, workgroup_size=block)
    es = pkg.HipES(parents, p - parents, **kw)
    es.track()
    es.set_survivors(k)
    want, pops = np.zeros(chunks, pkg.capi.CHUNK_RESULT_DTYPE), []
    for c in range(chunks):
        es.set_target_audio(tg[c])
        es.init_population(c)
        es.execute_generations(gens)
        bv, bs, bf, bg = es.best_ever()
        pop = es.read_population()
        r = want[c]
        r["generations_run"], r["best_ever_generation"], r["best_ever_fitness"], r["last_fitness"] = gens, bg, bf, pop[2][0]
        r["best_ever_values"][:d], r["best_ever_steps"][:d], r["last_values"][:d] = bv, bs, pop[0][0]
        pops.append(pop)
    es.close()
    b = pkg.HipBatch(2, parents, p - parents, **kw)
    b.track()
    b.set_survivors(k)
    b.queue_targets_audio(tg)
    got, _ = b.queue_run(0, gens, keep=keep)
    kept = b.queue_kept_population()
    b.close()
    assert len(got) == chunks
    for c in range(chunks):
        for name in ("generations_run", "best_ever_generation"):
            assert got[c][name] == want[c][name], (c, name, got[c][name], want[c][name])
        for name in ("best_ever_fitness", "last_fitness", "best_ever_values", "best_ever_steps", "last_values"):
            assert same_bits(got[c][name], want[c][name]), (c, name)
    for x, y in zip(kept, pops[keep]):
        assert same_bits(x, y)


# ---- (c) selection under such blocks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parents", [20, 30, 72])
def test_selection_plans_agree_under_block_24(pkg, parents):
    """breeding rows 24 > 20 parents, 24 < 30, 72 = 72; P = 4104 > 1024, so the fused loop selects (select_applies) and the
    second generation of AUTO and SPLITTERS ranks between the first one's splitters in one launch"""
    p, block = 4104, 24
    c = pkg.capi
    got = {}
    for label, plan, mode in (("auto", c.SELECT_AUTO, None), ("tiles", c.SELECT_TILES, None), ("splitters", c.SELECT_SPLITTERS, None),
                              ("full sort", c.SELECT_AUTO, c.SORT_FULL)):
        es = make(pkg, 0, parents, p - parents, block)
        es.set_select_plan(plan)
        if mode is not None:
            es.set_sort_mode(mode)
        es.init_population(0)
        es.execute_generations(2)
        got[label] = es.read_population()
        es.close()
    for label in ("auto", "tiles", "splitters"):
        for x, y, what in zip(got[label], got["full sort"], ("values", "steps", "fitness")):
            assert same_bits(x, y), (label, what, int(np.count_nonzero(bits(x) != bits(y))))
    f = got["full sort"][2]
    assert np.all(f[:-1] <= f[1:])


# ---- (d) step and value edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_mutate_step_and_value_edges(pkg, O, kind):
    """stage calls only: these genes are never synthesised"""
    d, p = DIMS[kind], vm.EDGE_ROWS
    v, s = vm.edge_population(d)
    es = make(pkg, kind, 1024, p - 1024, 32)
    for gen in (vm.SITE_GENERATION,) + vm.EDGE_GENERATIONS:
        es.write_population(v, s, np.zeros(p, np.float32))
        es.generation = gen
        es.mutate()
        gv, gs, _ = es.read_population()
        mv, ms = vm.mutate(v, s, O.mutate_words(p, d, vm.SEED, 0, gen), d)
        judge(gv, gs, mv, ms, part="edges", site="k_mutate", P=p, D=d, generation=gen)
        # what IEEE leaves no choice about, from the model's result
        zero, inf, nan = ms == 0.0, np.isinf(ms), np.isnan(ms)
        assert zero.any() and inf.any() and nan.any()
        assert np.all(gs[zero] == 0.0) and np.all(gs[inf] == ms[inf].astype(np.float32)) and np.all(np.isnan(gs[nan]))
        assert np.array_equal(np.isnan(gs), nan)
    es.close()


@pytest.mark.parametrize("name,kind,p,in_synth", vm.SITES, ids=SITE_IDS)
def test_finite_edges_through_the_sites(pkg, O, name, kind, p, in_synth):
    """steps 0 ... 3.0 and values in [-0.3, 1.7] only: what a synthesis kernel may be handed"""
    v, s = vm.edge_population(DIMS[kind], finite=True, rows=p)
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(s)) and s.max() <= 3.0 and v.min() >= -0.3 and v.max() <= np.float32(1.7)
    site_case(pkg, O, name, kind, p, in_synth, 0, v, s, "finite edges")


# ---- (e) counters -----------------------------------------------------------------------------------------------------------------
def init_words(O, p, d, gid_base, chunk):
    return np.array([[O.draw_word(vm.SEED, gid_base + i, chunk, j, O.TAG_INIT) for j in range(d)] for i in range(p)], np.uint32)


def test_counters_that_wrap_stage_kernels(pkg, O):
    """gid_base + i wraps 2^32 in the middle of the population; generations 2^32 - 1 and 2^31; chunk 2^32 - 1"""
    p, d, parents, block = vm.WRAP_P, 4, vm.SITE_PARENTS, vm.SITE_BLOCK
    es = make(pkg, 0, parents, p - parents, block, gid_base=vm.WRAP_GID)
    for chunk in (0, vm.EDGE_CHUNK):
        es.init_population(chunk)
        gv, gs, _ = es.read_population()
        mv, ms = vm.init(init_words(O, p, d, vm.WRAP_GID, chunk))
        assert same_bits(gv, mv) and same_bits(gs, ms), f"init_population({chunk:#x})"
    v, s = vm.site_population(p, d, 99)
    for gen in (vm.SITE_GENERATION,) + vm.EDGE_GENERATIONS:
        es.write_population(v, s, np.zeros(p, np.float32))
        es.generation = gen
        es.recombine(); es.mutate()
        gv, gs, _ = es.read_population()
        mv, ms = vm.generation(v, s, parents, block, O.mutate_words(p, d, vm.SEED, vm.WRAP_GID, gen))
        judge(gv, gs, mv, ms, part="counters", site="k_recombine + k_mutate", P=p, D=d, gid_base=vm.WRAP_GID, generation=gen)
    es.close()


@pytest.mark.parametrize("gen", vm.EDGE_GENERATIONS)
def test_counters_that_wrap_fused_loop(pkg, gen):
    """the sum in make_gene inside a synthesis kernel (k_synth_tp here): two fused generations from the edge generation -
    the second under the counter after it, 0 after 2^32 - 1 - equal two staged ones"""
    p, parents, block = vm.WRAP_P, vm.SITE_PARENTS, vm.SITE_BLOCK
    a = make(pkg, 0, parents, p - parents, block, gid_base=vm.WRAP_GID)
    b = make(pkg, 0, parents, p - parents, block, gid_base=vm.WRAP_GID)
    for e in (a, b):
        e.init_population(vm.EDGE_CHUNK)
        e.generation = gen
    a.execute_generations(2)
    staged_generation(b); staged_generation(b)
    assert a.generation == b.generation == (gen + 2) & M32
    for x, y in zip(a.read_population(), b.read_population()):
        assert same_bits(x, y)
    a.close(); b.close()


def test_counters_that_wrap_batch(pkg, O):
    """first_chunk_index 2^32 - 2 with four chunks (chunks 2^32 - 2, 2^32 - 1, 0, 1) and the wrapping gid_base: the
    initialised rows equal the model's, two generations equal a sequential context's"""
    kind, d, p, parents, block = 0, 4, vm.WRAP_P, vm.SITE_PARENTS, vm.SITE_BLOCK
    first, chunks = vm.BATCH_FIRST_CHUNK, vm.BATCH_CHUNKS
    tg = targets(chunks, N)
    kw = dict(synth_kind=kind, audio_log2=vm.N_LOG2, param_max=PMAX[kind], seed=vm.SEED, workgroup_size=block, gid_base=vm.WRAP_GID)
    b = pkg.HipBatch(chunks, parents, p - parents, **kw)
    b.set_target_audio(tg)
    b.init_population(first)
    for c in range(chunks):
        gv, gs, _ = b.read_population(c)
        mv, ms = vm.init(init_words(O, p, d, vm.WRAP_GID, (first + c) & M32))
        assert same_bits(gv, mv) and same_bits(gs, ms), f"chunk {c}"
    b.execute_generations(2)
    es = pkg.HipES(parents, p - parents, **kw)
    for c in range(chunks):
        es.set_target_audio(tg[c])
        es.init_population((first + c) & M32)
        es.execute_generations(2)
        for x, y in zip(b.read_population(c), es.read_population()):
            assert same_bits(x, y), f"chunk {c}"
    b.close(); es.close()
