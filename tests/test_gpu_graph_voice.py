"""The operator-graph voice on the device (SOTS_SYNTH_GRAPH: sots_create_graph, sots_batch_create_graph, k_synth_graph).

Synthesis is compared bit for bit with the NumPy model of the definition (tests/_graph_voice_model.py), which
tests/test_graph_voice_cpu.py pins to the oracle on the two graphs that restate a fixed voice.  Whole runs of those two
graphs are compared bit for bit with the fixed-voice contexts they restate: that holds the stand-alone variation launch,
the new kernel and the generation loop together against kernels that already pass.  Batch and queue are compared with
sequential tracked contexts of the same graph.
Covered: every operator count 2 to 8 (both block sizes, U = 8 and U = 4), fan-in up to 6, fan-out up to 7, 1 to 8 carriers;
workgroups of 1, 2, 3 and 4 wavefronts and a population that ends inside a transposed group of 8 rows; log2 N = 8, 9, 10 and
15; infinite and NaN modulator outputs and NaN phases from finite genes; the rest of a generation at D = 10, 14 and 16 is in
tests/test_gpu_graph_dims.py.  Left out: islands and continuous rendering (refused), non-finite genes, log2 N = 11 to 14,
the eight-wavefront experiment build, and a phase that is inf rather than NaN (tests/test_graph_voice_cpu.py says why)."""
import numpy as np
import pytest

from _graph_voice_model import GRAPHS, edge_rows, graph_synth, overflow_ranges, ranges
from _survivors_model import SEED, targets

pytestmark = pytest.mark.gpu

PMAX_2OP = [3520.0, 8.0, 3520.0, 1.0]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def graph_es(pkg, name, parents, offspring, log2n, pmin, pmax, block=32, **kw):
    return pkg.HipES(parents, offspring, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=log2n, param_min=pmin, param_max=pmax,
                     seed=SEED, workgroup_size=block, graph=pkg.capi.make_voice_graph(*GRAPHS[name]), **kw)


def synthesised(es, values):
    es.write_population(values=values)
    es.synthesise()
    return es.read_audio()


# ---- 1. synthesis against the model, bit for bit ------------------------------------------------------------------------------
# (parents, offspring, block): one wavefront; a partial one; two workgroups, the second ending inside a group of eight rows
# (100 = 64 + 4 x 8 + 4); several workgroups and a partial tile
POPULATIONS = {64: (32, 32, 32), 96: (32, 64, 32), 100: (50, 50, 50), 1056: (32, 1024, 32)}
_MODEL = {}


@pytest.fixture(scope="module")
def table(O):
    return O.wavetable()


def model_rows(name, n, table):
    """the largest population's rows and their audio, computed once per (graph, N): the smaller ones are its first rows"""
    key = (name, n)
    if key not in _MODEL:
        g = GRAPHS[name]
        pmin, pmax = ranges(g[0])  # negative minima (phases below 0) and an index range that overshoots W (the clamp)
        v = edge_rows(2 * g[0], max(POPULATIONS), 1000 + n)  # rows 0 and 1: all 0 and all 1
        _MODEL[key] = (pmin, pmax, v, graph_synth(g, v, pmin, pmax, n, table))
    return _MODEL[key]


@pytest.mark.parametrize("p", sorted(POPULATIONS))
@pytest.mark.parametrize("log2n", [8, 10])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_synthesis_equals_the_model(pkg, table, name, log2n, p):
    pmin, pmax, v, want = model_rows(name, 1 << log2n, table)
    parents, offspring, block = POPULATIONS[p]
    es = graph_es(pkg, name, parents, offspring, log2n, pmin, pmax, block=block)
    got = synthesised(es, v[:p])
    es.close()
    wrong = np.flatnonzero((bits(got) != bits(want[:p])).any(axis=1))
    assert wrong.size == 0, (name, log2n, p, wrong[:8], got[wrong[:1]], want[wrong[:1]])


def test_synthesis_of_a_population_that_loops_over_tiles(pkg, table):
    """P = 327 680 at N = 256: with at most 1024 rows per workgroup and 256 CUs a workgroup takes more than one tile.  The
    rows repeat with a prime period, so the model is computed for one period only"""
    p, period, n = 327680, 4099, 256
    pmin, pmax = ranges(2)
    base = edge_rows(4, period, 77)
    want = graph_synth(GRAPHS["2op"], base, pmin, pmax, n, table)
    idx = np.arange(p) % period
    es = graph_es(pkg, "2op", 32, p - 32, 8, pmin, pmax)
    got = synthesised(es, base[idx])
    es.close()
    wrong = np.flatnonzero((bits(got) != bits(want)[idx]).any(axis=1))
    assert wrong.size == 0, (wrong[:8], wrong.size)


def periodic_case(pkg, table, name, p, period, log2n, block, seed):
    """rows that repeat with a prime period, so that the model is computed for one period only"""
    g = GRAPHS[name]
    pmin, pmax = ranges(g[0])
    base = edge_rows(2 * g[0], period, seed)
    want = graph_synth(g, base, pmin, pmax, 1 << log2n, table)
    idx = np.arange(p) % period
    es = graph_es(pkg, name, block, p - block, log2n, pmin, pmax, block=block)
    got = synthesised(es, base[idx])
    es.close()
    wrong = np.flatnonzero((bits(got) != bits(want)[idx]).any(axis=1))
    assert wrong.size == 0, (name, p, wrong[:8], wrong.size)


@pytest.mark.parametrize("name", ["fan3", "stacks5"])  # samples in blocks of U = 8, and of U = 4
@pytest.mark.parametrize("p", [16392, 33032])
def test_synthesis_in_workgroups_of_two_and_three_wavefronts(pkg, table, name, p):
    """on 256 CUs P = 16 392 is a share of 65 rows per CU (two wavefronts, the second with one row in most workgroups) and
    P = 33 032 one of 130 (three): the wavefronts' tiles lie at stage_all + 1 and + 2 times kWave CH"""
    periodic_case(pkg, table, name, p, 1031, 8, 8, p)


@pytest.mark.parametrize("name,log2n,p", [("seven", 9, 96), ("chain3", 15, 64)])
def test_synthesis_at_other_lengths(pkg, table, name, log2n, p):
    """N = 512, and N = 32 768: the longest row, 1024 flushes of a tile"""
    g = GRAPHS[name]
    pmin, pmax = ranges(g[0])
    v = edge_rows(2 * g[0], p, 7 + log2n)
    want = graph_synth(g, v, pmin, pmax, 1 << log2n, table)
    es = graph_es(pkg, name, 32, p - 32, log2n, pmin, pmax)
    got = synthesised(es, v)
    es.close()
    wrong = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert wrong.size == 0, (name, log2n, wrong[:8])


@pytest.mark.parametrize("name", ["fan3", "dense8"])
def test_synthesis_with_an_infinite_modulator_level(pkg, table, name):
    """finite genes under overflow_ranges: operator 0's level is +inf, its output -inf or NaN, and the phases of what it
    modulates are NaN (tests/test_graph_voice_cpu.py shows that they occur).  The index is clamped on the float, so every
    such read is of entry 0 or W-1: nothing here is outside the definition.  Bit for bit; a NaN matches any NaN"""
    g = GRAPHS[name]
    pmin, pmax = overflow_ranges(g[0])
    v = edge_rows(2 * g[0], 96, 1256)
    want = graph_synth(g, v, pmin, pmax, 256, table)
    es = graph_es(pkg, name, 32, 64, 8, pmin, pmax)
    got = synthesised(es, v)
    es.close()
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    wrong = np.flatnonzero(~same.all(axis=1))
    assert wrong.size == 0, (name, wrong[:8], got[wrong[:1]], want[wrong[:1]])
    assert np.isfinite(want).all()


# ---- 2. whole runs against the fixed voices the anchors restate ---------------------------------------------------------------
@pytest.mark.parametrize("name,kind,parents,offspring", [("2op", 0, 512, 512), ("triple", 2, 128, 128)])
def test_fifty_generations_equal_the_fixed_voice(pkg, name, kind, parents, offspring):
    chains = GRAPHS[name][0] // 2
    fixed = pkg.HipES(parents, offspring, synth_kind=kind, audio_log2=10, param_max=PMAX_2OP + [0.0] * (4 * (chains - 1)), seed=SEED,
                      workgroup_size=32)
    graph = graph_es(pkg, name, parents, offspring, 10, None, PMAX_2OP * chains)  # the ranges repeated per chain
    target = targets(1, 1024)[0]
    for es in (fixed, graph):
        es.set_target_audio(target)
        es.init_population(0)
        es.execute_generations(50)
    want, got = fixed.read_population(), graph.read_population()
    assert fixed.generation == graph.generation == 50
    for what, a, b in zip(("values", "steps", "fitness"), got, want):
        assert same_bits(a, b), (name, what)
    fixed.close()
    graph.close()


# ---- 3. batch and queue against sequential tracked contexts -------------------------------------------------------------------
CHAIN = dict(name="chain3", parents=32, offspring=32, log2n=10, pmax=[3520.0, 8.0, 3520.0, 8.0, 3520.0, 1.0])
STALL = dict(target=None, stall=20, check_every=10)


def chain_batch(pkg, slots):
    b = pkg.HipBatch(slots, CHAIN["parents"], CHAIN["offspring"], synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=CHAIN["log2n"],
                     param_max=CHAIN["pmax"], seed=SEED, workgroup_size=32, graph=pkg.capi.make_voice_graph(*GRAPHS["chain3"]))
    b.track()
    return b


def chain_context(pkg):
    es = graph_es(pkg, CHAIN["name"], CHAIN["parents"], CHAIN["offspring"], CHAIN["log2n"], None, CHAIN["pmax"])
    es.track()
    return es


def test_three_chunks_in_a_batch_equal_three_contexts(pkg):
    tg = targets(3, 1 << CHAIN["log2n"])
    b = chain_batch(pkg, 3)
    b.set_target_audio(tg)
    b.init_population(0)
    b.execute_generations(40)
    bv, bs, bf, bg = b.best_ever()
    es = chain_context(pkg)
    for c in range(3):
        es.set_target_audio(tg[c])
        es.init_population(c)
        es.execute_generations(40)
        for what, a, w in zip(("values", "steps", "fitness"), b.read_population(c), es.read_population()):
            assert same_bits(a, w), (c, what)
        v, s, f, g = es.best_ever()
        assert same_bits(bv[c], v) and same_bits(bs[c], s) and same_bits(bf[c], f) and bg[c] == g, c
    es.close()
    b.close()


def test_three_chunks_through_a_two_slot_queue_equal_three_contexts(pkg):
    tg = targets(3, 1 << CHAIN["log2n"])
    b = chain_batch(pkg, 2)
    b.queue_targets_audio(tg)
    results, stats = b.queue_run(0, 200, **STALL)
    b.close()
    es = chain_context(pkg)
    d = es.D
    runs = []
    for c in range(3):
        es.set_target_audio(tg[c])
        es.init_population(c)
        run = es.execute_until(200, **STALL)
        v, s, f, g = es.best_ever()
        pop = es.read_population()
        r = results[c]
        assert (r["generations_run"], r["best_ever_generation"]) == (run, g), c
        assert same_bits(r["best_ever_fitness"], f) and same_bits(r["last_fitness"], pop[2][0]), c
        assert same_bits(r["best_ever_values"][:d], v) and same_bits(r["best_ever_steps"][:d], s) and same_bits(r["last_values"][:d], pop[0][0]), c
        runs.append(run)
    es.close()
    assert stats["slots"] == 2 and stats["chunk_generations"] == sum(runs)
    assert stats["global_generations"] == pkg.HipBatch.queue_makespan(np.asarray(runs, np.uint32), 2)


# ---- 4. survivors, rendering, what the voice refuses --------------------------------------------------------------------------
def test_with_one_survivor_the_best_fitness_never_rises(pkg, table):
    g = GRAPHS["two_mods"]
    pmax = [3520.0, 8.0, 3520.0, 8.0, 3520.0, 1.0]
    target = graph_synth(g, np.asarray([[0.11, 0.4, 0.07, 0.2, 0.25, 0.9]], np.float32), [0.0] * 6, pmax, 1024, table)[0]
    es = graph_es(pkg, "two_mods", 64, 192, 10, None, pmax)
    es.set_survivors(1)
    es.set_target_audio(target)
    es.init_population(0)
    best = []
    for _ in range(100):
        es.execute_generations(1)
        best.append(float(es.read_population()[2][0]))
    es.close()
    assert all(b <= a for a, b in zip(best, best[1:])), best
    assert best[-1] < best[0]


def test_overlap_add_rendering_equals_the_fixed_voice(pkg):
    fixed = pkg.HipES(32, 32, synth_kind=0, audio_log2=8, param_max=PMAX_2OP, seed=SEED, workgroup_size=32)
    graph = graph_es(pkg, "2op", 32, 32, 8, None, PMAX_2OP)
    v = edge_rows(4, 5, 9)[2:]  # three ordinary rows
    want, got = fixed.render_overlap_add(v, 128), graph.render_overlap_add(v, 128)
    fixed.close()
    graph.close()
    assert want.shape == got.shape == (2 * 128 + 256,) and same_bits(got, want)
    assert np.abs(want).max() > 0.01


def test_what_a_graph_context_refuses(pkg):
    hip = pkg.capi
    es = graph_es(pkg, "chain3", 32, 32, 8, None, CHAIN["pmax"])
    g = es.voice_graph()
    assert (g.num_operators, g.carriers, list(g.modulators)) == (3, 0b100, [0, 0b1, 0b10, 0, 0, 0, 0, 0])
    with pytest.raises(hip.SotsError) as e:
        es.set_synth_arithmetic(hip.ARITH_DEVICE_KERNELS)
    assert e.value.code == -1 and "the reference has no device kernel for the operator-graph voice" in str(e.value)
    es.set_synth_arithmetic(hip.ARITH_CPU_PATH)
    with pytest.raises(hip.SotsError) as e:
        es.render_continuous(edge_rows(6, 3, 1), 128)
    assert e.value.code == -1 and "sots_render_continuous: not for the operator-graph voice" in str(e.value)
    es.close()
    b = chain_batch(pkg, 2)
    with pytest.raises(hip.SotsError) as e:
        b.set_synth_arithmetic(hip.ARITH_DEVICE_KERNELS)
    assert e.value.code == -1 and "operator-graph voice" in str(e.value)
    b.close()
    fixed = pkg.HipES(32, 32, synth_kind=0, audio_log2=8, param_max=PMAX_2OP, seed=SEED, workgroup_size=32)
    with pytest.raises(hip.SotsError) as e:
        fixed.voice_graph()
    assert e.value.code == -5
    fixed.close()
