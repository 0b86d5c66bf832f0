"""The graph voice's time-parallel synthesis form on the device (k_synth_graph_tp; sots_set_graph_synth_form, DESIGN.md
4.20).  Every comparison is bit for bit, and every case asserts that `effective` is the form it means to test.

1. Synthesis under a forced TIME_PARALLEL against the NumPy model of the definition (tests/_graph_voice_model.py): all
   thirteen graphs, N = 256 (four blocks: fewer than the pipeline of chain8 and dense8 is deep, so fill and drain overlap),
   512 and 1024, N = 4096 for chain3; P = 1 (a one-row rendering: a population has at least two rows), 4, 5 (ends inside
   an evaluator's group of four), 37 and 1056 (a ragged last workgroup on 256 CUs); exactly capacity x CUs rows and one more;
   dense8 at P = 300, where a CU's share exceeds the capacity and the forced form takes several groups per workgroup.
2. TIME_PARALLEL against LANES on one context, switching the form between two sots_stage_synthesise calls: negative range
   minima, genes at 0 and 1, an infinite modulator level (NaN phases), every waveform code as a modulator and as a carrier.
3. Whole runs under AUTO, LANES and TIME_PARALLEL against each other and against the fixed voices the anchors restate.
4. Batch, queue with carried rows, overlap-add rendering: TIME_PARALLEL against LANES.
5. The choice rule."""
import numpy as np
import pytest

from _graph_voice_model import GRAPHS, edge_rows, graph_synth, overflow_ranges, ranges
from _survivors_model import SEED, targets

pytestmark = pytest.mark.gpu

PMAX_2OP = [3520.0, 8.0, 3520.0, 1.0]
AUTO, LANES, TIME = 0, 1, 2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def graph_es(pkg, name, parents, offspring, log2n, pmin, pmax, block=32, form=None, **kw):
    es = pkg.HipES(parents, offspring, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=log2n, param_min=pmin, param_max=pmax,
                   seed=SEED, workgroup_size=block, graph=pkg.capi.make_voice_graph(*GRAPHS[name]), **kw)
    if form is not None:
        es.set_graph_synth_form(form)
        assert es.graph_synth_form() == (form, form), (name, es.graph_synth_form())
    return es


def synthesised(es, values):
    es.write_population(values=values)
    es.synthesise()
    return es.read_audio()


def wrong_rows(got, want):
    return np.flatnonzero((bits(got) != bits(want)).any(axis=1))


@pytest.fixture(scope="module")
def table(O):
    return O.wavetable()


# ---- 1. forced TIME_PARALLEL against the model ---------------------------------------------------------------------------------
# (parents, offspring, block) of a population of P rows
POPULATIONS = {4: (1, 3, 1), 5: (1, 4, 1), 37: (1, 36, 1), 1056: (32, 1024, 32)}
_MODEL = {}


def model_rows(name, n, table):
    """the largest population's rows and their audio, once per (graph, N): the smaller ones are its first rows"""
    key = (name, n)
    if key not in _MODEL:
        g = GRAPHS[name]
        pmin, pmax = ranges(g[0])  # negative minima (the lower wrap) and an index range that overshoots W (the clamp)
        v = edge_rows(2 * g[0], max(POPULATIONS), 2000 + n)  # rows 0 and 1: all 0 and all 1
        _MODEL[key] = (pmin, pmax, v, graph_synth(g, v, pmin, pmax, n, table))
    return _MODEL[key]


@pytest.mark.parametrize("log2n", [8, 9, 10])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_forced_time_parallel_equals_the_model(pkg, table, name, log2n):
    pmin, pmax, v, want = model_rows(name, 1 << log2n, table)
    for p in sorted(POPULATIONS):
        parents, offspring, block = POPULATIONS[p]
        es = graph_es(pkg, name, parents, offspring, log2n, pmin, pmax, block=block, form=TIME)
        got = synthesised(es, v[:p])
        if p == 4:  # P = 1: one row rendered without a window is the row (the same context, one row per synthesis launch)
            one = es.render_overlap_add(v[2:3], 1 << log2n, windowed=False)
            assert same_bits(one, want[2]), (name, log2n, "one row")
        es.close()
        wrong = wrong_rows(got, want[:p])
        assert wrong.size == 0, (name, log2n, p, wrong[:8], got[wrong[:1]], want[wrong[:1]])


def test_forced_time_parallel_at_4096_samples(pkg, table):
    g = GRAPHS["chain3"]
    pmin, pmax = ranges(3)
    v = edge_rows(6, 37, 4096)
    want = graph_synth(g, v, pmin, pmax, 4096, table)
    es = graph_es(pkg, "chain3", 1, 36, 12, pmin, pmax, block=1, form=TIME)
    got = synthesised(es, v)
    es.close()
    assert wrong_rows(got, want).size == 0


def periodic_case(pkg, table, name, p, period, log2n, seed):
    """rows that repeat with a prime period, so that the model is computed for one period only"""
    g = GRAPHS[name]
    pmin, pmax = ranges(g[0])
    base = edge_rows(2 * g[0], period, seed)
    want = graph_synth(g, base, pmin, pmax, 1 << log2n, table)
    idx = np.arange(p) % period
    es = graph_es(pkg, name, 1, p - 1, log2n, pmin, pmax, block=1, form=TIME)
    got = synthesised(es, base[idx])
    es.close()
    wrong = wrong_rows(got, want[idx])
    assert wrong.size == 0, (name, p, wrong[:8], wrong.size)


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("name", ["2op", "fan3"])
def test_exactly_the_capacity_of_every_cu_and_one_row_more(pkg, table, name, extra):
    """capacity x CUs rows fill one group per workgroup; one row more and a CU's share exceeds the capacity: more groups
    than CUs, and a workgroup takes a second one"""
    cap, _ = pkg.capi.graph_time_parallel_capacity(pkg.capi.make_voice_graph(*GRAPHS[name]))
    probe = graph_es(pkg, name, 1, 1, 8, None, [1.0] * (2 * GRAPHS[name][0]), block=1)
    cus = probe.info().compute_units
    probe.close()
    periodic_case(pkg, table, name, cap * cus + extra, 211, 8, 31 + extra)


def test_a_share_beyond_the_capacity_takes_several_groups(pkg, table):
    """dense8 holds one individual per workgroup: P = 300 on 256 CUs is a share of 2"""
    assert pkg.capi.graph_time_parallel_capacity(pkg.capi.make_voice_graph(*GRAPHS["dense8"]))[0] == 1
    periodic_case(pkg, table, "dense8", 300, 97, 8, 300)


# ---- 2. TIME_PARALLEL against LANES on one context -----------------------------------------------------------------------------
def both_forms(es, values):
    """the audio of the same rows under LANES and under TIME_PARALLEL, the form switched between two synthesis calls"""
    es.write_population(values=values)
    out = []
    for form in (LANES, TIME):
        es.set_graph_synth_form(form)
        assert es.graph_synth_form() == (form, form)
        es.synthesise()
        out.append(es.read_audio())
    return out


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_the_forms_agree_with_negative_minima_and_genes_at_0_and_1(pkg, name):
    ops = GRAPHS[name][0]
    pmin, pmax = ranges(ops)
    v = edge_rows(2 * ops, 96, 17)
    v[2, ::2], v[3, 1::2], v[4, ::2], v[5, 1::2] = 0.0, 0.0, 1.0, 1.0  # every frequency / every level at an end of its range
    es = graph_es(pkg, name, 32, 64, 9, pmin, pmax)
    lanes, time = both_forms(es, v)
    es.close()
    assert wrong_rows(time, lanes).size == 0 and np.abs(lanes).max() > 0.01


@pytest.mark.parametrize("name", ["fan3", "dense8"])
def test_the_forms_agree_behind_an_infinite_modulator_level(pkg, table, name):
    """overflow_ranges: operator 0's level is +inf, the phases of what it modulates are NaN (tests/test_graph_voice_cpu.py
    shows that they occur); the audio stays finite, and equals the model's"""
    g = GRAPHS[name]
    pmin, pmax = overflow_ranges(g[0])
    v = edge_rows(2 * g[0], 96, 1256)
    es = graph_es(pkg, name, 32, 64, 8, pmin, pmax)
    lanes, time = both_forms(es, v)
    es.close()
    assert np.isfinite(lanes).all() and wrong_rows(time, lanes).size == 0
    assert wrong_rows(time, graph_synth(g, v, pmin, pmax, 256, table)).size == 0


@pytest.mark.parametrize("code", range(8))
def test_the_forms_agree_for_every_waveform_as_modulator_and_as_carrier(pkg, code):
    pmin, pmax = ranges(2)
    v = edge_rows(4, 37, 50 + code)
    es = graph_es(pkg, "2op", 1, 36, 9, pmin, pmax, block=1, waveforms=[code, code])
    lanes, time = both_forms(es, v)
    es.close()
    assert wrong_rows(time, lanes).size == 0 and np.abs(lanes).max() > 0.01
    # ... and with every other operator of a larger graph on another code
    ops = GRAPHS["seven"][0]
    pmin, pmax = ranges(ops)
    es = graph_es(pkg, "seven", 1, 36, 8, pmin, pmax, block=1, waveforms=[(code + j) % 8 for j in range(ops)])
    lanes, time = both_forms(es, edge_rows(2 * ops, 37, 60 + code))
    es.close()
    assert wrong_rows(time, lanes).size == 0


# ---- 3. whole runs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind,parents,offspring", [("2op", 0, 256, 768), ("triple", 2, 128, 128)])
def test_fifty_generations_equal_under_every_form_and_equal_the_fixed_voice(pkg, name, kind, parents, offspring):
    chains = GRAPHS[name][0] // 2
    cap, _ = pkg.capi.graph_time_parallel_capacity(pkg.capi.make_voice_graph(*GRAPHS[name]))
    fixed = pkg.HipES(parents, offspring, synth_kind=kind, audio_log2=10, param_max=PMAX_2OP + [0.0] * (4 * (chains - 1)), seed=SEED,
                      workgroup_size=32)
    assert parents + offspring <= cap * fixed.info().compute_units  # one group per workgroup
    runs = [fixed] + [graph_es(pkg, name, parents, offspring, 10, None, PMAX_2OP * chains) for _ in (AUTO, LANES, TIME)]
    for es, form in zip(runs[1:], (AUTO, LANES, TIME)):
        es.set_graph_synth_form(form)
        assert es.graph_synth_form()[0] == form and (form == AUTO or es.graph_synth_form()[1] == form)
    target = targets(1, 1024)[0]
    for es in runs:
        es.set_target_audio(target)
        es.init_population(0)
        es.execute_generations(50)
    want = fixed.read_population()
    for es, form in zip(runs[1:], ("auto", "lanes", "time")):
        assert es.generation == 50
        for what, a, b in zip(("values", "steps", "fitness"), es.read_population(), want):
            assert same_bits(a, b), (name, form, what)
    for es in runs:
        es.close()


# ---- 4. batch, queue, rendering ------------------------------------------------------------------------------------------------
CHAIN = dict(parents=16, offspring=16, log2n=10, pmax=[3520.0, 8.0, 3520.0, 8.0, 3520.0, 1.0])
STALL = dict(target=None, stall=20, check_every=10)
RESULT_FIELDS = ("generations_run", "best_ever_generation", "best_ever_fitness", "last_fitness", "best_ever_values", "best_ever_steps",
                 "last_values")


def chain_batch(pkg, slots, form):
    b = pkg.HipBatch(slots, CHAIN["parents"], CHAIN["offspring"], synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=CHAIN["log2n"],
                     param_max=CHAIN["pmax"], seed=SEED, workgroup_size=16, graph=pkg.capi.make_voice_graph(*GRAPHS["chain3"]))
    b.track()
    b.set_survivors(1)
    b.set_graph_synth_form(form)
    assert b.graph_synth_form() == (form, form)
    return b


def test_eight_chunks_in_a_batch_equal_under_both_forms(pkg):
    tg = targets(8, 1 << CHAIN["log2n"])
    seen = []
    for form in (LANES, TIME):
        b = chain_batch(pkg, 8, form)
        b.set_target_audio(tg)
        b.init_population(0)
        b.execute_generations(40)
        seen.append(([b.read_population(c) for c in range(8)], b.best_ever()))
        b.close()
    (pops_l, best_l), (pops_t, best_t) = seen
    for c in range(8):
        for what, a, w in zip(("values", "steps", "fitness"), pops_t[c], pops_l[c]):
            assert same_bits(a, w), (c, what)
    for what, a, w in zip(("values", "steps", "fitness"), best_t[:3], best_l[:3]):
        assert same_bits(a, w), what
    assert np.array_equal(best_t[3], best_l[3]) and np.all(np.isfinite(best_l[2]))


def test_a_two_slot_queue_with_two_carried_rows_equals_under_both_forms(pkg):
    tg = targets(5, 1 << CHAIN["log2n"])
    seen = []
    for form in (LANES, TIME):
        b = chain_batch(pkg, 2, form)
        b.queue_set_carry(2, 2)
        b.queue_targets_audio(tg)
        seen.append(b.queue_run(0, 100, **STALL))
        b.close()
    (want, stats_l), (got, stats_t) = seen
    assert len(got) == len(want) == 5 and stats_l == stats_t
    for k in range(5):
        for field in RESULT_FIELDS:
            assert same_bits(got[k][field], want[k][field]) if got[k][field].dtype.kind == "f" else got[k][field] == want[k][field], (k, field)


def test_overlap_add_rendering_of_seven_rows_equals_under_both_forms(pkg):
    es = graph_es(pkg, "two_mods", 32, 32, 10, None, CHAIN["pmax"])
    v = edge_rows(6, 9, 9)[2:]  # seven ordinary rows
    out = []
    for form in (LANES, TIME):
        es.set_graph_synth_form(form)
        assert es.graph_synth_form() == (form, form)
        out.append(es.render_overlap_add(v, 256))
    es.close()
    assert out[0].shape == (6 * 256 + 1024,) and same_bits(out[1], out[0]) and np.abs(out[0]).max() > 0.01


# ---- 5. the choice rule --------------------------------------------------------------------------------------------------------
def test_auto_takes_the_small_population_and_leaves_the_large_one(pkg):
    small = graph_es(pkg, "2op", 256, 768, 10, None, PMAX_2OP)
    assert small.graph_synth_form() == (AUTO, TIME)
    small.close()
    large = graph_es(pkg, "2op", 16384, 49152, 8, None, PMAX_2OP)
    assert large.graph_synth_form() == (AUTO, LANES)
    large.set_graph_synth_form(TIME)  # forced: any population
    assert large.graph_synth_form() == (TIME, TIME)
    large.close()


def test_feedback_and_feedback_genes_keep_the_lane_form(pkg):
    hip = pkg.capi
    es = graph_es(pkg, "2op", 256, 768, 10, None, PMAX_2OP)
    for form in (AUTO, TIME):
        es.set_graph_synth_form(form)
        assert es.graph_synth_form() == (form, TIME)
        es.set_voice_feedback([0.0, 0.5])
        assert es.graph_synth_form() == (form, LANES)
        es.set_voice_feedback([0.0, 0.0])
        assert es.graph_synth_form() == (form, TIME)
    with pytest.raises(hip.SotsError) as e:
        es.set_graph_synth_form(3)
    assert e.value.code == -1 and "3 is not a form" in str(e.value) and es.graph_synth_form() == (TIME, TIME)
    es.close()
    genes = pkg.HipES(256, 768, synth_kind=hip.SYNTH_GRAPH, audio_log2=10, param_max=PMAX_2OP + [2.0], seed=SEED, workgroup_size=32,
                      graph=hip.make_voice_graph(*GRAPHS["2op"]), feedback_genes=[1])
    for form in (AUTO, LANES, TIME):
        genes.set_graph_synth_form(form)
        assert genes.graph_synth_form() == (form, LANES)
    genes.close()
    fixed = pkg.HipES(32, 32, synth_kind=0, audio_log2=8, param_max=PMAX_2OP, seed=SEED, workgroup_size=32)
    for call in (lambda: fixed.set_graph_synth_form(LANES), fixed.graph_synth_form):
        with pytest.raises(hip.SotsError) as e:
            call()
        assert e.value.code == -5 and "graph synthesis form: the handle runs a fixed voice (synth_kind 0)" in str(e.value)
    fixed.close()
    b = pkg.HipBatch(2, 16, 16, synth_kind=0, audio_log2=8, param_max=PMAX_2OP, seed=SEED, workgroup_size=16)
    with pytest.raises(hip.SotsError) as e:
        b.set_graph_synth_form(TIME)
    assert e.value.code == -5 and "fixed voice" in str(e.value)
    b.close()


def test_setting_the_form_in_a_tracked_run_clears_nothing(pkg):
    """twenty generations, the form changed after ten: best-ever record, history and population are those of a run that never
    touched the form"""
    runs = []
    for switch in (False, True):
        es = graph_es(pkg, "chain3", 32, 32, 10, None, CHAIN["pmax"])
        es.set_target_audio(targets(1, 1024)[0])
        es.init_population(0)
        es.track(history_every=1, capacity=32)
        es.execute_generations(10)
        if switch:
            before = (es.best_ever(), es.history(with_taken=True))
            es.set_graph_synth_form(TIME if es.graph_synth_form()[1] == LANES else LANES)
            after = (es.best_ever(), es.history(with_taken=True))
            for a, b in zip(before[0], after[0]):
                assert same_bits(a, b) if isinstance(a, np.ndarray) else a == b
            assert before[1][1] == after[1][1] == 10 and before[1][0].tobytes() == after[1][0].tobytes()
        es.execute_generations(10)
        runs.append((es.read_population(), es.best_ever(), es.history(with_taken=True)))
        es.close()
    (pop_a, best_a, hist_a), (pop_b, best_b, hist_b) = runs
    for a, b in zip(pop_a, pop_b):
        assert same_bits(a, b)
    assert same_bits(best_a[0], best_b[0]) and same_bits(best_a[2], best_b[2]) and best_a[3] == best_b[3]
    assert hist_a[1] == hist_b[1] == 20 and hist_a[0].tobytes() == hist_b[0].tobytes()
