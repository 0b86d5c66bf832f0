"""The graph voice's operator waveforms on the device (sots_set_voice_waveforms, sots_batch_set_voice_waveforms, the shaped
form of k_synth_graph).

Every comparison is bit for bit against the NumPy model of the definition (tests/_graph_waveforms_model.py), which
tests/test_graph_waveforms_cpu.py pins to the all-sine model and through it to the oracle; a NaN matches any NaN.  Whole
runs are compared with other routes through the same library: stage by stage against the generation loop, batch and queue
against sequential tracked contexts, the renderer against tests/_render_model.py's accumulation of the model's rows."""
import numpy as np
import pytest

import _render_model as R
from _graph_waveforms_model import (GRAPHS, SAW, SQUARE, W, additive_synth_waves, edge_rows, graph_synth_waves, overflow_ranges,
                                    ranges)
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


def rotated(ops, r):
    return [(j + r) % 8 for j in range(ops)]


# ---- 1. synthesis on the base graphs ------------------------------------------------------------------------------------------
BASE = ["2op", "chain3", "two_mods", "additive", "fan3", "stacks5", "seven", "dense8", "additive8"]
ROTATIONS = [0, 3, 6]
# (parents, offspring, block): one wavefront; a population that ends inside a group of eight rows (100 = 64 + 4 x 8 + 4)
POPULATIONS = {64: (32, 32, 32), 100: (50, 50, 50)}
_MODEL = {}


def model_rows(name, r, n, table):
    """100 rows and their audio, once per (graph, rotation, N): the 64 are its first rows"""
    key = (name, r, n)
    if key not in _MODEL:
        g = GRAPHS[name]
        pmin, pmax = ranges(g[0])  # negative minima (phases below 0) and an index range that overshoots W (the clamp)
        v = edge_rows(2 * g[0], 100, 2000 + n)
        _MODEL[key] = (pmin, pmax, v, graph_synth_waves(g, rotated(g[0], r), v, pmin, pmax, n, table))
    return _MODEL[key]


def test_the_cases_cover_every_code_in_every_role():
    """among the graphs whose samples go in blocks of 8 (up to four operators) and among those of blocks of 4, every code
    sits on a modulated operator, an unmodulated one, a modulator and a carrier"""
    for wide in (True, False):
        roles = {"modulated": set(), "unmodulated": set(), "modulator": set(), "carrier": set()}
        for name in BASE:
            ops, mods, carriers = GRAPHS[name]
            if (ops <= 4) != wide:
                continue
            for r in ROTATIONS:
                for j, w in enumerate(rotated(ops, r)):
                    roles["modulated" if mods[j] else "unmodulated"].add(w)
                    roles["carrier" if carriers >> j & 1 else "modulator"].add(w)
        for role, codes in roles.items():
            assert codes == set(range(8)), (wide, role, codes)


@pytest.mark.parametrize("p", sorted(POPULATIONS))
@pytest.mark.parametrize("r", ROTATIONS)
@pytest.mark.parametrize("name", BASE)
def test_synthesis_equals_the_model(pkg, table, name, r, p):
    pmin, pmax, v, want = model_rows(name, r, 256, table)
    parents, offspring, block = POPULATIONS[p]
    es = graph_es(pkg, name, parents, offspring, 8, pmin, pmax, block=block, waveforms=rotated(GRAPHS[name][0], r))
    got = synthesised(es, v[:p])
    es.close()
    wrong = wrong_rows(got, want[:p])
    assert wrong.size == 0, (name, r, p, wrong[:8], got[wrong[:1]], want[wrong[:1]])


def test_synthesis_at_n_1024(pkg, table):
    pmin, pmax, v, want = model_rows("stacks5", 3, 1024, table)
    es = graph_es(pkg, "stacks5", 50, 50, 10, pmin, pmax, block=50, waveforms=rotated(5, 3))
    got = synthesised(es, v)
    es.close()
    wrong = wrong_rows(got, want)
    assert wrong.size == 0, (wrong[:8], got[wrong[:1]], want[wrong[:1]])


# ---- 2. the table walk --------------------------------------------------------------------------------------------------------
def test_every_region_of_every_shape_is_read(pkg, table):
    """additive8 with codes 0..7 at N = 32768, frequencies 0 .. 2 x 44100 / 32768 Hz: a phase advances by up to two entries a
    sample, so it walks the table between zero and two times - every region of every shape, both sides of W/4 and W/2"""
    waves = list(range(8))
    pmin, pmax = [0.0] * 16, [2 * 44100 / 32768, 1.0] * 8
    v = edge_rows(16, 64, 3000)
    hit = np.zeros((8, W), bool)
    want = additive_synth_waves(waves, v, pmin, pmax, 1 << 15, table, hit)
    for w in waves:
        for edge in (W // 4, W // 2, 3 * W // 4):
            assert hit[w, edge - 2:edge + 2].all(), (w, edge)
        assert hit[w].reshape(64, -1).any(axis=1).all() and hit[w, W - 2:].any(), w
    es = graph_es(pkg, "additive8", 32, 32, 15, pmin, pmax, waveforms=waves)
    assert es.voice_waveforms() == waves
    got = synthesised(es, v)
    es.close()
    wrong = wrong_rows(got, want)
    assert wrong.size == 0, (wrong[:8], np.flatnonzero(bits(got[wrong[0]]) != bits(want[wrong[0]]))[:4] if wrong.size else None)
    assert np.isfinite(want).all() and np.abs(want).max() > 0.1


# ---- 3. non-finite values -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fan3", "dense8"])
def test_square_and_saw_behind_an_infinite_modulator_level(pkg, table, name):
    """overflow_ranges: operator 0's level is +inf, what it modulates has NaN phases, and a NaN phase reads index 0 - where
    SQUARE gives +1 and SAW gives -1, whatever the table holds there"""
    g = GRAPHS[name]
    ops, mods, _ = g
    waves = [0] * ops
    modulated = [j for j in range(ops) if mods[j] & 1]
    waves[modulated[0]] = SQUARE
    waves[modulated[-1]] = SAW if len(modulated) > 1 else SQUARE
    if len(modulated) == 1:  # fan3: operator 3 alone is modulated - once SQUARE, once SAW
        cases = [[0, 0, 0, SQUARE], [0, 0, 0, SAW]]
    else:
        cases = [waves]
    pmin, pmax = overflow_ranges(ops)
    v = edge_rows(2 * ops, 96, 1256)
    for codes in cases:
        want = graph_synth_waves(g, codes, v, pmin, pmax, 256, table)
        es = graph_es(pkg, name, 32, 64, 8, pmin, pmax, waveforms=codes)
        got = synthesised(es, v)
        es.close()
        wrong = wrong_rows(got, want)
        assert wrong.size == 0, (name, codes, wrong[:8], got[wrong[:1]], want[wrong[:1]])
    if name == "fan3":  # the carrier's own output at a NaN phase: +1 a_3 and -1 a_3, from sample 1 on, in the overflowed rows
        a3 = (np.asarray(pmin, np.float32) + v * (np.asarray(pmax, np.float32) - np.asarray(pmin, np.float32)))[:, 7]
        sq = graph_synth_waves(g, cases[0], v, pmin, pmax, 256, table)
        sw = graph_synth_waves(g, cases[1], v, pmin, pmax, 256, table)
        nan_rows = np.flatnonzero((v[:, 0] * v[:, 1] > 0.5) & (v[:, 0] > 0.3))
        assert nan_rows.size > 3
        assert all(same_bits(sq[r, 2:], np.full(254, a3[r], np.float32)) and same_bits(sw[r, 2:], np.full(254, -a3[r], np.float32))
                   for r in nan_rows)


# ---- 4. workgroups of three wavefronts ----------------------------------------------------------------------------------------
def test_shaped_synthesis_in_workgroups_of_three_wavefronts(pkg, table):
    """P = 33 032 on 256 CUs is a share of 130 rows per CU; the rows repeat with the prime period 1031"""
    p, period, waves = 33032, 1031, [5, 2, 7, 4]
    g = GRAPHS["fan3"]
    pmin, pmax = ranges(4)
    base = edge_rows(8, period, p)
    want = graph_synth_waves(g, waves, base, pmin, pmax, 256, table)
    idx = np.arange(p) % period
    es = graph_es(pkg, "fan3", 8, p - 8, 8, pmin, pmax, block=8, waveforms=waves)
    got = synthesised(es, base[idx])
    es.close()
    wrong = wrong_rows(got, want[idx])
    assert wrong.size == 0, (wrong[:8], wrong.size)


# ---- 5. setting and resetting -------------------------------------------------------------------------------------------------
def test_set_get_reset_and_refusals(pkg, table):
    hip = pkg.capi
    g = GRAPHS["chain3"]
    pmin, pmax = ranges(3)
    v = edge_rows(6, 64, 5000)
    never = graph_es(pkg, "chain3", 32, 32, 8, pmin, pmax)
    assert never.voice_waveforms() == [0, 0, 0]
    plain = synthesised(never, v)
    never.close()
    es = graph_es(pkg, "chain3", 32, 32, 8, pmin, pmax)
    es.set_voice_waveforms(["saw", "half", hip.WAVE_ABS_EVEN])
    assert es.voice_waveforms() == [7, 1, 5]
    shaped = synthesised(es, v)
    assert wrong_rows(shaped, graph_synth_waves(g, [7, 1, 5], v, pmin, pmax, 256, table)).size == 0
    assert not same_bits(shaped, plain)
    refusals = [([7, 8, 5], -1, "voice waveforms: code 8 of operator 1 is not a waveform (0..7)"),
                ([7, 1], -1, "voice waveforms: 2 codes for a graph of 3 operators"),
                ([7, 1, 5, 0], -1, "voice waveforms: 4 codes for a graph of 3 operators")]
    for codes, rc, text in refusals:
        with pytest.raises(hip.SotsError) as e:
            es.set_voice_waveforms(codes)
        assert e.value.code == rc and text in str(e.value), (codes, str(e.value))
        assert es.voice_waveforms() == [7, 1, 5] and same_bits(synthesised(es, v), shaped), codes
    assert es.L.sots_set_voice_waveforms(es._h, None, 3) == -1
    assert es.L.sots_last_error(es._h).decode() == "voice waveforms: null codes with a count of 3"
    assert es.voice_waveforms() == [7, 1, 5] and same_bits(synthesised(es, v), shaped)
    for reset in ([0, 0, 0], None):
        es.set_voice_waveforms([2, 2, 2])
        es.set_voice_waveforms(reset)
        assert es.voice_waveforms() == [0, 0, 0] and same_bits(synthesised(es, v), plain), reset
    es.close()
    # a context and a batch of a fixed voice
    fixed = pkg.HipES(32, 32, synth_kind=0, audio_log2=8, param_max=[3520.0, 8.0, 3520.0, 1.0], seed=SEED, workgroup_size=32)
    before = synthesised(fixed, v[:, :4])
    for call in (lambda: fixed.set_voice_waveforms([1, 1]), lambda: fixed.set_voice_waveforms(None), fixed.voice_waveforms):
        with pytest.raises(hip.SotsError) as e:
            call()
        assert e.value.code == -5 and "voice waveforms: the handle runs a fixed voice (synth_kind 0)" in str(e.value)
    assert same_bits(synthesised(fixed, v[:, :4]), before)
    fixed.close()
    b = pkg.HipBatch(2, 32, 32, synth_kind=0, audio_log2=8, param_max=[3520.0, 8.0, 3520.0, 1.0], seed=SEED, workgroup_size=32)
    with pytest.raises(hip.SotsError) as e:
        b.set_voice_waveforms([1, 1])
    assert e.value.code == -5
    b.close()


# ---- 6. whole runs ------------------------------------------------------------------------------------------------------------
CHAIN = dict(parents=32, offspring=32, log2n=8, pmax=[3520.0, 8.0, 3520.0, 8.0, 3520.0, 1.0], waves=[6, 3, 1])
STALL = dict(target=None, stall=20, check_every=10)


def chain_context(pkg, waves=CHAIN["waves"], track=True):
    es = graph_es(pkg, "chain3", CHAIN["parents"], CHAIN["offspring"], CHAIN["log2n"], None, CHAIN["pmax"], waveforms=waves)
    if track:
        es.track()
    return es


def chain_batch(pkg, slots, survivors=0):
    b = pkg.HipBatch(slots, CHAIN["parents"], CHAIN["offspring"], synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=CHAIN["log2n"],
                     param_max=CHAIN["pmax"], seed=SEED, workgroup_size=32, graph=pkg.capi.make_voice_graph(*GRAPHS["chain3"]),
                     waveforms=CHAIN["waves"])
    assert b.voice_waveforms() == CHAIN["waves"]
    b.track()
    b.set_survivors(survivors)
    return b


def test_twenty_generations_stage_by_stage_equal_the_loop(pkg, table):
    tg = targets(1, 256)[0]
    loop, staged, sine = chain_context(pkg, track=False), chain_context(pkg, track=False), chain_context(pkg, None, track=False)
    for es in (loop, staged, sine):
        es.set_target_audio(tg)
        es.init_population(0)
    loop.execute_generations(20)
    sine.execute_generations(20)
    for _ in range(20):
        staged.recombine(); staged.mutate()
        staged.synthesise(); staged.window(); staged.fft(); staged.fitness(); staged.sort(); staged.rotate()
    got, want, other = staged.read_population(), loop.read_population(), sine.read_population()
    assert loop.generation == staged.generation == 20
    for what, a, b in zip(("values", "steps", "fitness"), got, want):
        assert same_bits(a, b), what
    assert not same_bits(want[2], other[2]), "the waveforms did not reach the generation loop"
    # the loop's last synthesis is the model's audio of the rows it evaluated
    v = want[0]
    assert wrong_rows(synthesised(loop, v), graph_synth_waves(GRAPHS["chain3"], CHAIN["waves"], v, [0.0] * 6, CHAIN["pmax"], 256, table)).size == 0
    for es in (loop, staged, sine):
        es.close()


def test_three_chunks_in_a_batch_equal_three_contexts(pkg):
    tg = targets(3, 256)
    b = chain_batch(pkg, 3)
    b.set_target_audio(tg)
    b.init_population(0)
    b.execute_generations(30)
    bv, bs, bf, bg = b.best_ever()
    es, sine = chain_context(pkg), chain_context(pkg, None)
    for c in range(3):
        es.set_target_audio(tg[c])
        es.init_population(c)
        es.execute_generations(30)
        for what, a, w in zip(("values", "steps", "fitness"), b.read_population(c), es.read_population()):
            assert same_bits(a, w), (c, what)
        v, s, f, g = es.best_ever()
        assert same_bits(bv[c], v) and same_bits(bs[c], s) and same_bits(bf[c], f) and bg[c] == g, c
    sine.set_target_audio(tg[2])
    sine.init_population(2)
    sine.execute_generations(30)
    assert not same_bits(sine.read_population()[2], es.read_population()[2]), "the waveforms did not reach the batch's twin"
    es.close(); sine.close(); b.close()


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


@pytest.mark.parametrize("rows", [0, 1], ids=["plain", "carry1"])
def test_three_chunks_through_a_two_slot_queue_equal_three_contexts(pkg, rows):
    """one survivor; with one carried row, segments of two chunks (chunk 1 starts from chunk 0's best-ever record)"""
    max_g, segment = 100, 2
    tg = targets(3, 256)
    es = chain_context(pkg)
    es.set_survivors(1)
    want = sequential_reference(pkg, es, tg, max_g, STALL, rows, segment)
    es.close()
    b = chain_batch(pkg, 2, survivors=1)
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


def test_overlap_add_rendering_equals_the_accumulated_model_rows(pkg, O, table):
    n, hop = 256, 128
    v = R.unit_rows(3, 6, 17)
    rows = graph_synth_waves(GRAPHS["chain3"], CHAIN["waves"], v, [0.0] * 6, CHAIN["pmax"], n, table)
    es = chain_context(pkg, track=False)
    for windowed in (True, False):
        got = es.render_overlap_add(v, hop, windowed=windowed)
        want = R.overlap_add(rows, hop, R.window32(O, n) if windowed else None)
        assert got.shape == want.shape == (2 * hop + n,) and same_bits(got, want), windowed
    es.close()
    assert np.abs(rows).max() > 0.01


# ---- 7. a change in mid-run ---------------------------------------------------------------------------------------------------
def test_a_change_after_ten_generations(pkg):
    """P = 4096 (the selection applies): after the change the record reads as cleared and the run goes on as a fresh context's
    that was given the same population, steps, counter and codes - under every select plan (stale splitters would show),
    and the plans agree afterwards"""
    parents, offspring, after = 1024, 3072, [4, 0, 7]
    tg = targets(1, 256)[0]

    def context(plan, waves):
        es = graph_es(pkg, "chain3", parents, offspring, 8, None, CHAIN["pmax"], waveforms=waves)
        es.set_select_plan(plan)
        es.set_target_audio(tg)
        es.track(history_every=1, capacity=64)
        return es

    ends = []
    for plan in (pkg.capi.SELECT_AUTO, pkg.capi.SELECT_TILES, pkg.capi.SELECT_SPLITTERS):
        es = context(plan, CHAIN["waves"])
        es.init_population(0)
        es.execute_generations(10)
        assert es.best_ever()[3] > 0 and len(es.history()) == 10
        es.set_voice_waveforms(after)
        v, s, f, g = es.best_ever()
        hist, taken = es.history(with_taken=True)
        assert np.isposinf(f) and g == 0 and not v.any() and not s.any() and taken == 0 and len(hist) == 0, plan
        assert es.generation == 10 and es.voice_waveforms() == after
        pop = es.read_population()
        es.execute_generations(10)
        fresh = context(plan, after)
        fresh.write_population(*pop)
        fresh.generation = 10
        fresh.execute_generations(10)
        for what, a, b in zip(("values", "steps", "fitness"), es.read_population(), fresh.read_population()):
            assert same_bits(a, b), (plan, what)
        (v, s, f, g), (fv, fs, ff, fg) = es.best_ever(), fresh.best_ever()
        assert same_bits(v, fv) and same_bits(s, fs) and same_bits(f, ff) and g == fg and g > 10, plan
        ends.append(es.read_population())
        es.close(); fresh.close()
    for other in ends[1:]:
        for what, a, b in zip(("values", "steps", "fitness"), ends[0], other):
            assert same_bits(a, b), what
