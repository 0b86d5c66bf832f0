"""The graph voice's per-operator feedback on the device (sots_set_voice_feedback, sots_batch_set_voice_feedback, the feedback
form of k_synth_graph).

Every comparison is bit for bit against the NumPy model of the definition (tests/_graph_feedback_model.py), which
tests/test_graph_feedback_cpu.py pins to the model of the waveforms and through it to the oracle; a NaN matches any NaN.
Whole runs are compared with other routes through the same library: stage by stage against the generation loop, batch and
queue against sequential tracked contexts, the renderer against tests/_render_model.py's accumulation of the model's rows."""
import numpy as np
import pytest

import _render_model as R
from _graph_feedback_model import GRAPHS, SAW, SQUARE, edge_rows, graph_synth_feedback, graph_synth_waves, overflow_ranges, ranges
from _survivors_model import SEED, targets

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def wrong_rows(got, want):
    """rows that differ in a bit, a NaN matching any NaN"""
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    return np.flatnonzero(~same.all(axis=1))


@pytest.fixture(scope="module")
def table(O):
    return O.wavetable()


def graph_es(pkg, name, parents, offspring, log2n, pmin, pmax, block=32, **kw):
    return pkg.HipES(parents, offspring, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=log2n, param_min=pmin, param_max=pmax,
                     seed=SEED, workgroup_size=block, graph=pkg.capi.make_voice_graph(*GRAPHS[name]), **kw)


def synthesised(es, values):
    es.write_population(values=values)
    es.synthesise()
    return es.read_audio()


# ---- 1. synthesis: who feeds back --------------------------------------------------------------------------------------------
def fed(name, who):
    """the operators of the graph that feed back in a case"""
    ops, mods, carriers = GRAPHS[name]
    if who == "plain_modulator":  # unmodulated, not heard
        return [j for j in range(ops) if not mods[j] and not carriers >> j & 1]
    if who == "modulated":
        return [j for j in range(ops) if mods[j]]
    if who == "carrier":
        return [j for j in range(ops) if carriers >> j & 1]
    if who == "all":
        return list(range(ops))
    if who == "beside":  # every other operator, the rest with an index of zero
        return list(range(0, ops, 2))
    raise ValueError(who)


# one graph whose samples go in blocks of 8 (up to four operators) and one of blocks of 4 for each kind; 2 ... 8 operators
CASES = [("2op", "plain_modulator"), ("stacks5", "plain_modulator"),
         ("chain3", "modulated"), ("chain8", "modulated"),
         ("one_mod_two_carriers", "carrier"), ("seven", "carrier"),
         ("fan3", "all"), ("dense8", "all"),
         ("two_mods", "beside"), ("triple", "beside")]
INDICES = [0.25, 1.0, 2.0]
CODES = {"sine": None, "mixed": 6}  # the rotation 6, 7, 0, 1, ...: SQUARE and SAW, the shapes that read no table, come first
# (parents, offspring, block): one wavefront; a population that ends inside a group of eight rows and a second wavefront
POPULATIONS = {64: (32, 32, 32), 100: (50, 50, 50)}
_MODEL = {}


def codes_of(ops, rotation):
    return [0] * ops if rotation is None else [(j + rotation) % 8 for j in range(ops)]


def beta_of(name, who, index):
    ops = GRAPHS[name][0]
    on = fed(name, who)
    return [index if j in on else 0.0 for j in range(ops)]


def model_rows(name, who, index, codes, n, table):
    """100 rows and their audio, once per case: the 64 are its first rows"""
    key = (name, who, index, codes, n)
    if key not in _MODEL:
        g = GRAPHS[name]
        pmin, pmax = ranges(g[0])  # negative minima (phases below 0) and an index range that overshoots W (the clamp)
        v = edge_rows(2 * g[0], 100, 4000 + n)
        _MODEL[key] = (pmin, pmax, v, graph_synth_feedback(g, codes_of(g[0], CODES[codes]), beta_of(name, who, index), v, pmin, pmax, n, table))
    return _MODEL[key]


def test_the_cases_cover_every_operator_count_and_kind():
    assert {GRAPHS[name][0] for name, _ in CASES} == set(range(2, 9))
    for who in ("plain_modulator", "modulated", "carrier", "all", "beside"):
        widths = {GRAPHS[name][0] <= 4 for name, w in CASES if w == who}
        assert widths == {True, False}, who
    for name, who in CASES:
        on = fed(name, who)
        assert on and (who == "all" or len(on) < GRAPHS[name][0]), (name, who)
    mixed = codes_of(2, CODES["mixed"])
    assert SQUARE in mixed and SAW in mixed


@pytest.mark.parametrize("codes", sorted(CODES))
@pytest.mark.parametrize("index", INDICES)
@pytest.mark.parametrize("name,who", CASES)
def test_synthesis_equals_the_model(pkg, table, name, who, index, codes):
    """N = 256: 8 flushes of 32 samples, 32 or 64 blocks - h1 and h2 cross every kind of boundary"""
    pmin, pmax, v, want = model_rows(name, who, index, codes, 256, table)
    ops = GRAPHS[name][0]
    for p, (parents, offspring, block) in sorted(POPULATIONS.items()):
        es = graph_es(pkg, name, parents, offspring, 8, pmin, pmax, block=block, waveforms=codes_of(ops, CODES[codes]),
                      feedback=beta_of(name, who, index))
        got = synthesised(es, v[:p])
        es.close()
        wrong = wrong_rows(got, want[:p])
        assert wrong.size == 0, (name, who, index, codes, p, wrong[:8], got[wrong[:1]], want[wrong[:1]])
    assert not same_bits(want, graph_synth_waves(GRAPHS[name], codes_of(ops, CODES[codes]), v, pmin, pmax, 256, table)), "the case feeds nothing back"


# ---- 2. workgroups of three wavefronts; a workgroup that loops over tiles ------------------------------------------------------
@pytest.mark.parametrize("p", [33032, 65600], ids=["three_wavefronts", "tile_loop"])
def test_feedback_in_wide_workgroups(pkg, table, p):
    """P = 33 032 on 256 CUs is a share of 130 rows per CU: three wavefronts.  P = 65 600 is more than 256 workgroups of 256
    rows: a workgroup goes on to a second tile, and h1 and h2 start again at +0 with every row.  The rows repeat with the
    prime period 1031"""
    period, waves, beta = 1031, [5, 0, 7, 4], [1.0, 0.0, 0.25, 2.0]
    g = GRAPHS["fan3"]
    pmin, pmax = ranges(4)
    base = edge_rows(8, period, 33032)
    want = graph_synth_feedback(g, waves, beta, base, pmin, pmax, 256, table)
    idx = np.arange(p) % period
    es = graph_es(pkg, "fan3", 8, p - 8, 8, pmin, pmax, block=8, waveforms=waves, feedback=beta)
    got = synthesised(es, base[idx])
    es.close()
    wrong = wrong_rows(got, want[idx])
    assert wrong.size == 0, (wrong[:8], wrong.size)


# ---- 3. non-finite and out-of-range phases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fan3", "dense8"])
def test_nan_and_out_of_range_phases_go_to_the_clamp(pkg, table, name):
    """overflow_ranges: operator 0's level is +inf, what it modulates has NaN phases, and so has the offset phase z"""
    g = GRAPHS[name]
    ops = g[0]
    pmin, pmax = overflow_ranges(ops)
    v = edge_rows(2 * ops, 96, 1257)
    for waves, beta in ((codes_of(ops, None), [1.0] * ops), (codes_of(ops, 6), [2.0 if j % 2 else 0.25 for j in range(ops)])):
        want = graph_synth_feedback(g, waves, beta, v, pmin, pmax, 256, table)
        es = graph_es(pkg, name, 32, 64, 8, pmin, pmax, waveforms=waves, feedback=beta)
        got = synthesised(es, v)
        es.close()
        wrong = wrong_rows(got, want)
        assert wrong.size == 0, (name, waves, beta, wrong[:8], got[wrong[:1]], want[wrong[:1]])
    assert (v[:, 0] * v[:, 1] > 0.5).sum() > 3


# ---- 4. setting and resetting -------------------------------------------------------------------------------------------------
def test_set_get_reset_and_refusals(pkg, table):
    hip = pkg.capi
    g = GRAPHS["chain3"]
    pmin, pmax = ranges(3)
    v = edge_rows(6, 64, 5001)
    never = graph_es(pkg, "chain3", 32, 32, 8, pmin, pmax)
    assert never.voice_feedback() == [0.0, 0.0, 0.0]
    plain = synthesised(never, v)
    never.close()
    es = graph_es(pkg, "chain3", 32, 32, 8, pmin, pmax)
    es.set_voice_feedback([0.25, 0, 2])
    assert es.voice_feedback() == [0.25, 0.0, 2.0]
    fedback = synthesised(es, v)
    assert wrong_rows(fedback, graph_synth_feedback(g, [0, 0, 0], [0.25, 0.0, 2.0], v, pmin, pmax, 256, table)).size == 0
    assert not same_bits(fedback, plain)
    refusals = [([0.25, 2.5, 0], -1, "voice feedback: index 2.5 of operator 1 is outside 0..2"),
                ([0.25, 0, -1.0], -1, "voice feedback: index -1 of operator 2 is outside 0..2"),
                ([float("inf"), 0, 0], -1, "voice feedback: index inf of operator 0 is outside 0..2"),
                ([0, float("nan"), 0], -1, "nan of operator 1 is outside 0..2"),
                ([0.25, 1], -1, "voice feedback: 2 indices for a graph of 3 operators"),
                ([0.25, 1, 1, 0], -1, "voice feedback: 4 indices for a graph of 3 operators")]
    for index, rc, text in refusals:
        with pytest.raises(hip.SotsError) as e:
            es.set_voice_feedback(index)
        assert e.value.code == rc and text in str(e.value), (index, str(e.value))
        assert es.voice_feedback() == [0.25, 0.0, 2.0] and same_bits(synthesised(es, v), fedback), index
    assert es.L.sots_set_voice_feedback(es._h, None, 3) == -1
    assert es.L.sots_last_error(es._h).decode() == "voice feedback: null indices with a count of 3"
    assert es.voice_feedback() == [0.25, 0.0, 2.0] and same_bits(synthesised(es, v), fedback)
    # the waveforms and the feedback are two settings: either leaves the other
    es.set_voice_waveforms([7, 1, 5])
    assert es.voice_feedback() == [0.25, 0.0, 2.0]
    assert wrong_rows(synthesised(es, v), graph_synth_feedback(g, [7, 1, 5], [0.25, 0.0, 2.0], v, pmin, pmax, 256, table)).size == 0
    es.set_voice_feedback(None)
    assert es.voice_waveforms() == [7, 1, 5]
    assert wrong_rows(synthesised(es, v), graph_synth_waves(g, [7, 1, 5], v, pmin, pmax, 256, table)).size == 0
    es.set_voice_waveforms(None)
    for reset in ([0, 0, 0], [-0.0, 0.0, -0.0], None):
        es.set_voice_feedback([1, 1, 1])
        es.set_voice_feedback(reset)
        got = es.voice_feedback()
        assert got == [0.0, 0.0, 0.0] and not np.signbit(got).any() and same_bits(synthesised(es, v), plain), reset
    es.close()
    # a context and a batch of a fixed voice
    fixed = pkg.HipES(32, 32, synth_kind=0, audio_log2=8, param_max=[3520.0, 8.0, 3520.0, 1.0], seed=SEED, workgroup_size=32)
    before = synthesised(fixed, v[:, :4])
    for call in (lambda: fixed.set_voice_feedback([1, 1]), lambda: fixed.set_voice_feedback(None), fixed.voice_feedback):
        with pytest.raises(hip.SotsError) as e:
            call()
        assert e.value.code == -5 and "voice feedback: the handle runs a fixed voice (synth_kind 0)" in str(e.value)
    assert same_bits(synthesised(fixed, v[:, :4]), before)
    fixed.close()
    b = pkg.HipBatch(2, 32, 32, synth_kind=0, audio_log2=8, param_max=[3520.0, 8.0, 3520.0, 1.0], seed=SEED, workgroup_size=32)
    with pytest.raises(hip.SotsError) as e:
        b.set_voice_feedback([1, 1])
    assert e.value.code == -5
    b.close()


# ---- 5. whole runs: P = 64, N = 256, a 2-operator and a 5-operator graph --------------------------------------------------------
RUNS = {"2op": dict(pmax=[3520.0, 8.0, 3520.0, 1.0], waves=None, beta=[1.0, 0.5]),
        "stacks5": dict(pmax=[3520.0, 8.0, 3520.0, 8.0, 3520.0, 1.0, 3520.0, 8.0, 3520.0, 1.0], waves=[0, 7, 0, 1, 6], beta=[0.5, 0.0, 1.5, 2.0, 0.25])}
STALL = dict(target=None, stall=20, check_every=10)


def run_context(pkg, name, feedback=True, track=True):
    r = RUNS[name]
    es = graph_es(pkg, name, 32, 32, 8, None, r["pmax"], waveforms=r["waves"], feedback=r["beta"] if feedback else None)
    if track:
        es.track()
    return es


def run_batch(pkg, name, slots, survivors=0):
    r = RUNS[name]
    b = pkg.HipBatch(slots, 32, 32, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=8, param_max=r["pmax"], seed=SEED, workgroup_size=32,
                     graph=pkg.capi.make_voice_graph(*GRAPHS[name]), waveforms=r["waves"], feedback=r["beta"])
    assert b.voice_feedback() == r["beta"]
    b.track()
    b.set_survivors(survivors)
    return b


@pytest.mark.parametrize("name", sorted(RUNS))
def test_five_generations_stage_by_stage_equal_the_loop(pkg, table, name):
    r = RUNS[name]
    tg = targets(1, 256)[0]
    loop, staged, off = run_context(pkg, name, track=False), run_context(pkg, name, track=False), run_context(pkg, name, False, track=False)
    for es in (loop, staged, off):
        es.set_target_audio(tg)
        es.init_population(0)
    loop.execute_generations(5)
    off.execute_generations(5)
    for _ in range(5):
        staged.recombine(); staged.mutate()
        staged.synthesise(); staged.window(); staged.fft(); staged.fitness(); staged.sort(); staged.rotate()
    got, want, other = staged.read_population(), loop.read_population(), off.read_population()
    assert loop.generation == staged.generation == 5
    for what, a, b in zip(("values", "steps", "fitness"), got, want):
        assert same_bits(a, b), what
    assert not same_bits(want[2], other[2]), "the feedback did not reach the generation loop"
    # the loop's last synthesis is the model's audio of the rows it evaluated
    v = want[0]
    ops = GRAPHS[name][0]
    model = graph_synth_feedback(GRAPHS[name], codes_of(ops, None) if r["waves"] is None else r["waves"], r["beta"], v, [0.0] * (2 * ops), r["pmax"], 256, table)
    assert wrong_rows(synthesised(loop, v), model).size == 0
    for es in (loop, staged, off):
        es.close()


@pytest.mark.parametrize("name", sorted(RUNS))
def test_set_then_reset_continues_as_a_run_that_never_set_it(pkg, name):
    """... and a successful call clears the run record"""
    tg = targets(1, 256)[0]
    es, never = run_context(pkg, name, False), run_context(pkg, name, False)
    for e in (es, never):
        e.set_target_audio(tg)
        e.init_population(0)
        e.execute_generations(5)
    assert es.best_ever()[3] > 0
    es.set_voice_feedback(RUNS[name]["beta"])
    v, s, f, g = es.best_ever()
    assert np.isposinf(f) and g == 0 and not v.any() and not s.any() and es.generation == 5
    es.set_voice_feedback(None)
    es.execute_generations(5)
    never.execute_generations(5)
    for what, a, b in zip(("values", "steps", "fitness"), es.read_population(), never.read_population()):
        assert same_bits(a, b), what
    es.close(); never.close()


def sequential_reference(pkg, es, tg, max_g, rule, rows, segment):
    """the sequence include/sots_hip.h gives as the definition of the queue with carried rows, on one tracked context"""
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


@pytest.mark.parametrize("name", sorted(RUNS))
def test_a_batch_and_a_two_slot_queue_with_a_carried_row_equal_sequential_contexts(pkg, name):
    tg = targets(3, 256)
    # the batch: three chunks side by side against three runs of one context
    b = run_batch(pkg, name, 3)
    b.set_target_audio(tg)
    b.init_population(0)
    b.execute_generations(10)
    bv, bs, bf, bg = b.best_ever()
    es, off = run_context(pkg, name), run_context(pkg, name, False)
    for c in range(3):
        es.set_target_audio(tg[c])
        es.init_population(c)
        es.execute_generations(10)
        for what, a, w in zip(("values", "steps", "fitness"), b.read_population(c), es.read_population()):
            assert same_bits(a, w), (c, what)
        v, s, f, g = es.best_ever()
        assert same_bits(bv[c], v) and same_bits(bs[c], s) and same_bits(bf[c], f) and bg[c] == g, c
    off.set_target_audio(tg[2])
    off.init_population(2)
    off.execute_generations(10)
    assert not same_bits(off.read_population()[2], es.read_population()[2]), "the feedback did not reach the batch's twin"
    es.close(); off.close(); b.close()
    # the queue: two slots, one survivor, one carried row, segments of two chunks
    max_g, segment, rows = 60, 2, 1
    es = run_context(pkg, name)
    es.set_survivors(1)
    want = sequential_reference(pkg, es, tg, max_g, STALL, rows, segment)
    es.close()
    b = run_batch(pkg, name, 2, survivors=1)
    b.queue_set_carry(rows, segment)
    b.queue_targets_audio(tg)
    got, stats = b.queue_run(0, max_g, **STALL)
    b.close()
    assert len(got) == 3
    for k in range(3):
        for field in ("generations_run", "best_ever_generation"):
            assert got[k][field] == want[k][field], (k, field, got[k][field], want[k][field])
        for field in ("best_ever_fitness", "last_fitness", "best_ever_values", "best_ever_steps", "last_values"):
            assert same_bits(got[k][field], want[k][field]), (k, field, got[k][field], want[k][field])
    assert stats["slots"] == 2 and stats["chunk_generations"] == int(want["generations_run"].sum())


@pytest.mark.parametrize("name", sorted(RUNS))
def test_overlap_add_rendering_equals_the_accumulated_model_rows(pkg, O, table, name):
    n, hop = 256, 128
    r = RUNS[name]
    ops = GRAPHS[name][0]
    v = R.unit_rows(3, 2 * ops, 17)
    rows = graph_synth_feedback(GRAPHS[name], codes_of(ops, None) if r["waves"] is None else r["waves"], r["beta"], v, [0.0] * (2 * ops), r["pmax"], n, table)
    es = run_context(pkg, name, track=False)
    for windowed in (True, False):
        got = es.render_overlap_add(v, hop, windowed=windowed)
        want = R.overlap_add(rows, hop, R.window32(O, n) if windowed else None)
        assert got.shape == want.shape == (2 * hop + n,) and same_bits(got, want), windowed
    es.close()
    assert np.abs(rows).max() > 0.01
