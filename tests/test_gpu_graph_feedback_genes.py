"""Feedback indices as genes on the device (sots_create_graph_genes, sots_batch_create_graph_genes, the gene form of
k_synth_graph).

Synthesis is compared bit for bit with the NumPy model of the definition (tests/_graph_feedback_genes_model.py), which
tests/test_graph_feedback_genes_cpu.py pins to the model of the fixed setting; a NaN matches any NaN.  The anchor is
checked against a context of the fixed setting, byte for byte.  These are the first rows of an odd width (D = 5 and 15):
initialisation, variation, the sorts, the selection plans and the run record are judged at those widths with the helpers
that tests/test_gpu_graph_dims.py uses.  Whole runs are compared with other routes through the same library."""
import numpy as np
import pytest

import _render_model as R
import _variation_model as vm
from _graph_feedback_genes_model import (GRAPHS, dims, edge_gene_rows, edge_rows, effective_beta, gene_operators, gene_ranges, graph_synth_feedback,
                                         graph_synth_genes, with_beta)
from _survivors_model import SEED, targets
from test_gpu_parity import fitness_pattern, sort_case
from test_gpu_run_record import check_best_ever, check_history
from test_gpu_select_splitters import prime, select_and_check
from test_gpu_variation import init_words, judge, staged_generation

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


def gene_es(pkg, name, mask, parents, offspring, log2n, pmin, pmax, block=32, **kw):
    es = pkg.HipES(parents, offspring, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=log2n, param_min=pmin, param_max=pmax,
                   seed=SEED, workgroup_size=block, graph=pkg.capi.make_voice_graph(*GRAPHS[name]), feedback_genes=mask, **kw)
    assert es.D == dims(GRAPHS[name][0], mask) and es.voice_feedback_genes() == mask
    return es


def synthesised(es, values):
    es.write_population(values=values)
    es.synthesise()
    return es.read_audio()


def codes_of(ops, rotation):
    return [0] * ops if rotation is None else [(j + rotation) % 8 for j in range(ops)]


# ---- 1. synthesis equals the model ------------------------------------------------------------------------------------------------
# (graph, mask, fixed indices): the carrier's gene (D = 5); both genes (D = 6); five genes (D = 15); one gene operator beside
# one operator of a fixed index and one without feedback (D = 7)
CASES = {"2op_carrier": ("2op", 0b10, [0.0, 0.0]),
         "2op_both": ("2op", 0b11, [0.0, 0.0]),
         "stacks5_all": ("stacks5", 0b11111, [0.0] * 5),
         "chain3_gene_beside_fixed": ("chain3", 0b010, [0.5, 0.0, 0.0])}
CODES = {"sine": None, "mixed": 6}  # the rotation 6, 7, 0, 1, ... of tests/test_gpu_graph_feedback.py
# (parents, offspring, block): one wavefront; a population that ends inside a group of eight rows of a second wavefront
POPULATIONS = {64: (32, 32, 32), 100: (50, 50, 50)}


def test_the_cases_are_those_of_the_definition():
    assert [dims(GRAPHS[g][0], m) for g, m, _ in CASES.values()] == [5, 6, 15, 7]
    g, m, beta = CASES["chain3_gene_beside_fixed"]
    assert gene_operators(3, m) == [1] and sum(b != 0 for b in beta) == 1 and beta[1] == 0


@pytest.mark.parametrize("codes", sorted(CODES))
@pytest.mark.parametrize("case", sorted(CASES))
def test_synthesis_equals_the_model(pkg, table, case, codes):
    """N = 256: 8 flushes of 32 samples; gene ranges [0, 2], so every row has its own beta, rows 0 and 1 the bounds"""
    name, mask, beta = CASES[case]
    g = GRAPHS[name]
    ops = g[0]
    pmin, pmax = gene_ranges(ops, mask)
    waves = codes_of(ops, CODES[codes])
    v = edge_rows(dims(ops, mask), 100, 4300 + ops)
    want = graph_synth_genes(g, waves, beta, mask, v, pmin, pmax, 256, table)
    for p, (parents, offspring, block) in sorted(POPULATIONS.items()):
        es = gene_es(pkg, name, mask, parents, offspring, 8, pmin, pmax, block=block, waveforms=waves, feedback=beta)
        got = synthesised(es, v[:p])
        es.close()
        wrong = wrong_rows(got, want[:p])
        assert wrong.size == 0, (case, codes, p, wrong[:8], got[wrong[:1]], want[wrong[:1]])
    # the genes are read: the same rows with every gene at 0 sound different
    silent = v.copy()
    silent[:, 2 * ops:] = 0.0
    assert not same_bits(want, graph_synth_genes(g, waves, beta, mask, silent, pmin, pmax, 256, table))


def test_genes_in_wide_workgroups(pkg, table):
    """P = 33 032 on 256 CUs is a share of 130 rows per CU: three wavefronts per workgroup, as in
    tests/test_gpu_graph_feedback.py.  The rows repeat with the prime period 1031"""
    period, p = 1031, 33032
    name, mask, beta = CASES["stacks5_all"]
    g = GRAPHS[name]
    waves = codes_of(5, 6)
    pmin, pmax = gene_ranges(5, mask)
    base = edge_rows(15, period, p)
    want = graph_synth_genes(g, waves, beta, mask, base, pmin, pmax, 256, table)
    idx = np.arange(p) % period
    es = gene_es(pkg, name, mask, 8, p - 8, 8, pmin, pmax, block=8, waveforms=waves)
    got = synthesised(es, base[idx])
    es.close()
    wrong = wrong_rows(got, want[idx])
    assert wrong.size == 0, (wrong[:8], wrong.size)


# ---- 2. the anchor ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", [0.25, 1.0, 2.0])
@pytest.mark.parametrize("name,mask", [("2op", 0b10), ("stacks5", 0b11111), ("one_mod_two_carriers", 0b110)])
def test_rows_of_a_constant_index_equal_the_fixed_setting(pkg, name, mask, index):
    """the audio of a context of sots_create_graph with sots_set_voice_feedback = index on the masked operators, byte for byte"""
    g = GRAPHS[name]
    ops = g[0]
    pmin, pmax = gene_ranges(ops, mask)
    waves = codes_of(ops, 6)
    plain = edge_rows(2 * ops, 64, 4400 + ops)
    fixed = pkg.HipES(32, 32, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=8, param_min=pmin[:2 * ops], param_max=pmax[:2 * ops], seed=SEED,
                      workgroup_size=32, graph=pkg.capi.make_voice_graph(*g), waveforms=waves,
                      feedback=[index if mask >> j & 1 else 0.0 for j in range(ops)])
    want = synthesised(fixed, plain)
    fixed.close()
    es = gene_es(pkg, name, mask, 32, 32, 8, pmin, pmax, waveforms=waves)
    got = synthesised(es, with_beta(plain, ops, mask, index))
    es.close()
    assert got.tobytes() == want.tobytes(), (name, index)
    assert np.abs(want).max() > 0.01


# ---- 3. the edge rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["2op_carrier", "stacks5_all"])
def test_edge_rows_go_to_the_clamp(pkg, table, case):
    """v = -0.5, 1.5, NaN and both infinities in every column.  The genes' range is [0.25, 1.75]: -0.5 scales to -0.5 (beta
    +0, the chain running), 1.5 to 2.5 (beta 2)"""
    name, mask, beta = CASES[case]
    g = GRAPHS[name]
    ops, d = g[0], dims(g[0], mask)
    pmin, pmax = gene_ranges(ops, mask, lo=0.25, hi=1.75)
    v = edge_gene_rows(d, 4500 + d, rows=96)
    scaled = np.float32(0.25) + v[:, 2 * ops:] * (np.float32(1.75) - np.float32(0.25))
    eff = effective_beta(scaled)
    assert (eff == 0).any() and (eff == 2).any() and np.isnan(scaled).any() and (scaled > 2).any() and (scaled < 0).any()
    for waves in (codes_of(ops, None), codes_of(ops, 6)):
        want = graph_synth_genes(g, waves, beta, mask, v, pmin, pmax, 256, table)
        es = gene_es(pkg, name, mask, 32, 64, 8, pmin, pmax, waveforms=waves)
        got = synthesised(es, v)
        es.close()
        wrong = wrong_rows(got, want)
        assert wrong.size == 0, (case, waves, wrong[:8], v[wrong[:1]], got[wrong[:1]], want[wrong[:1]])


# ---- 4. settings and refusals on a live handle --------------------------------------------------------------------------------------
def test_setting_getters_and_refusals(pkg, table):
    hip = pkg.capi
    g = GRAPHS["chain3"]
    mask = 0b010
    pmin, pmax = gene_ranges(3, mask)
    v = edge_rows(7, 64, 4600)
    es = gene_es(pkg, "chain3", mask, 32, 32, 8, pmin, pmax)
    assert es.voice_feedback() == [0.0, 0.0, 0.0]
    es.set_voice_feedback([0.5, 0, 2])
    assert es.voice_feedback() == [0.5, 0.0, 2.0] and es.voice_feedback_genes() == mask
    before = synthesised(es, v)
    assert wrong_rows(before, graph_synth_genes(g, [0, 0, 0], [0.5, 0.0, 2.0], mask, v, pmin, pmax, 256, table)).size == 0
    with pytest.raises(hip.SotsError) as e:
        es.set_voice_feedback([0.5, 0.25, 2])
    assert e.value.code == -1
    assert "voice feedback: index 0.25 for operator 1, whose index is a gene (feedback_genes 0x2): only 0 can be set" in str(e.value)
    assert es.voice_feedback() == [0.5, 0.0, 2.0] and same_bits(synthesised(es, v), before)
    # both renderers that take beta from the context
    rows = R.unit_rows(3, 7, 17)
    for call, who in ((es.render_graph_continuous, "sots_render_graph_continuous"), (es.render_graph_feedback, "sots_render_graph_feedback")):
        with pytest.raises(hip.SotsError) as e:
            call(rows, 128)
        assert e.value.code == -5
        assert (who + ": the feedback indices of operators 0x2 are genes (sots_create_graph_genes): every row has its own; "
                "sots_render_overlap_add renders such a voice") in str(e.value)
    es.close()
    # mask 0 through the new entry point is sots_create_graph
    pmin4, pmax4 = pmin[:6], pmax[:6]
    zero = gene_es(pkg, "chain3", 0, 32, 32, 8, pmin4, pmax4, feedback=[0.5, 0.25, 2])
    old = pkg.HipES(32, 32, synth_kind=hip.SYNTH_GRAPH, audio_log2=8, param_min=pmin4, param_max=pmax4, seed=SEED, workgroup_size=32,
                    graph=hip.make_voice_graph(*g), feedback=[0.5, 0.25, 2])
    assert zero.D == 6 and zero.voice_feedback_genes() == 0 and old.voice_feedback_genes() == 0
    assert zero.voice_feedback() == [0.5, 0.25, 2.0]
    assert synthesised(zero, v[:, :6]).tobytes() == synthesised(old, v[:, :6]).tobytes()
    assert zero.render_graph_feedback(rows[:, :6], 128).tobytes() == old.render_graph_feedback(rows[:, :6], 128).tobytes()
    zero.close(); old.close()
    # a context and a batch of a fixed voice
    fixed = pkg.HipES(32, 32, synth_kind=0, audio_log2=8, param_max=[3520.0, 8.0, 3520.0, 1.0], seed=SEED, workgroup_size=32)
    with pytest.raises(hip.SotsError) as e:
        fixed.voice_feedback_genes()
    assert e.value.code == -5 and "voice feedback genes: the handle runs a fixed voice (synth_kind 0)" in str(e.value)
    fixed.close()
    b = pkg.HipBatch(2, 32, 32, synth_kind=0, audio_log2=8, param_max=[3520.0, 8.0, 3520.0, 1.0], seed=SEED, workgroup_size=32)
    with pytest.raises(hip.SotsError) as e:
        b.voice_feedback_genes()
    assert e.value.code == -5
    b.close()


# ---- 5. odd widths outside synthesis: D = 5 and 15 ------------------------------------------------------------------------------------
ODD = {5: ("2op", 0b10), 15: ("stacks5", 0b11111)}
WIDTHS = sorted(ODD)


def pmax_of(d):
    """frequencies up to 3520 Hz, modulation indices up to 8, carrier levels up to 1, feedback indices up to 2"""
    name, mask = ODD[d]
    ops, _, carriers = GRAPHS[name]
    out = []
    for j in range(ops):
        out += [3520.0, 1.0 if carriers >> j & 1 else 8.0]
    return out + [2.0] * (d - 2 * ops)


def odd_context(pkg, d, parents, offspring, block=32, log2n=vm.N_LOG2, slots=0, target=True, survivors=0, generation=None, **kw):
    name, mask = ODD[d]
    args = dict(synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=log2n, param_max=pmax_of(d), seed=vm.SEED, workgroup_size=block,
                graph=pkg.capi.make_voice_graph(*GRAPHS[name]), feedback_genes=mask, **kw)
    if slots:
        b = pkg.HipBatch(slots, parents, offspring, **args)
        assert b.D == d and b.voice_feedback_genes() == mask
        b.track()
        b.set_survivors(survivors)
        return b
    es = pkg.HipES(parents, offspring, **args)
    assert es.D == d
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


@pytest.mark.parametrize("d", WIDTHS)
def test_init_population(pkg, O, d):
    p = 96
    es = odd_context(pkg, d, 32, 64, target=False)
    for chunk in (0, vm.EDGE_CHUNK):
        es.init_population(chunk)
        gv, gs, _ = es.read_population()
        mv, ms = vm.init(init_words(O, p, d, 0, chunk))
        assert same_bits(gv, mv) and same_bits(gs, ms), f"init_population({chunk:#x})"
    es.close()


@pytest.mark.parametrize("k", (0, 1))
@pytest.mark.parametrize("d", WIDTHS)
def test_one_generation(pkg, O, d, k):
    """the staged pre-sort population equals the model of variation, and one fused generation equals the staged one"""
    p = 768
    parents, block, gen = vm.SITE_PARENTS, vm.SITE_BLOCK, vm.SITE_GENERATION
    v, s = vm.site_population(p, d, p + d)
    zero = np.zeros(p, np.float32)
    a = odd_context(pkg, d, parents, p - parents, block=block, survivors=k, generation=gen)
    b = odd_context(pkg, d, parents, p - parents, block=block, survivors=k, generation=gen)
    for e in (a, b):
        e.write_population(v, s, zero)
    pv, ps = staged_generation(b)
    a.execute_generations(1)
    fused, staged = a.read_population(), b.read_population()
    a.close(); b.close()
    mv, ms = vm.generation(v, s, parents, block, O.mutate_words(p, d, vm.SEED, 0, gen), k)
    judge(pv, ps, mv, ms, part="site", site=f"k_recombine_mutate<graph genes D={d}>", P=p, D=d, block=block, parents=parents, survivors=k)
    if k:
        assert same_bits(pv[:k], v[:k]) and same_bits(ps[:k], s[:k]), "a survivor changed"
    for x, y, label in zip(fused, staged, ("values", "steps", "fitness")):
        assert same_bits(x, y), (label, int(np.count_nonzero(x != y)))
    assert np.all(np.isfinite(fused[2]))


@pytest.mark.parametrize("parents,p,block", [(40, 1000, 40), (50, 2050, 50)], ids=["one_workgroup", "tiles"])
@pytest.mark.parametrize("d", WIDTHS)
def test_sort_matches_the_stable_order(pkg, O, d, parents, p, block):
    """rows of 2 D + 1 = 11 and 31 floats through both sorts: ties, NaN, inf and signed zeros in the fitness"""
    es = odd_context(pkg, d, parents, p - parents, block=block, target=False)
    es.set_sort_mode(pkg.capi.SORT_FULL)
    rng, v, s = random_rows(p, d, p + d)
    f = sort_case(p, rng)
    f[::97] = f[5]
    es.write_population(v, s, f)
    es.sort(); es.rotate()
    gv, gs, gf = es.read_population()
    es.close()
    perm = O.sort_perm(f)
    assert np.array_equal(gf, f[perm], equal_nan=True)
    assert np.array_equal(gv, v[perm]) and np.array_equal(gs, s[perm])


@pytest.mark.parametrize("plan", [1, 2], ids=["tiles", "splitters"])
@pytest.mark.parametrize("d", WIDTHS)
def test_select_places_exactly_the_rows_recombination_reads(pkg, O, d, plan):
    parents, p, pattern = 1024, 4096, "few_values"
    es = odd_context(pkg, d, parents, p - parents, log2n=9, target=False)
    es.set_select_plan(plan)
    rng, v, s = random_rows(p, d, parents + d)
    f = fitness_pattern(pattern, p, rng)
    if plan == pkg.capi.SELECT_SPLITTERS:
        prime(pkg, es, fitness_pattern(pattern, p, rng))
    select_and_check(pkg, O, es, parents, f, v, s)
    es.close()


@pytest.mark.parametrize("d", WIDTHS)
def test_three_generations_under_auto_tiles_and_splitters_are_equal(pkg, d):
    parents, p = 1024, 4096
    runs = []
    for plan in (pkg.capi.SELECT_AUTO, pkg.capi.SELECT_TILES, pkg.capi.SELECT_SPLITTERS):
        es = odd_context(pkg, d, parents, p - parents)
        es.set_select_plan(plan)
        es.init_population(0)
        es.execute_generations(3)
        runs.append(es.read_population())
        es.close()
    for other in runs[1:]:
        for x, y, label in zip(runs[0], other, ("values", "steps", "fitness")):
            assert same_bits(x, y), label
    assert np.all(np.isfinite(runs[0][2])) and np.all(np.diff(runs[0][2]) >= 0)


@pytest.mark.parametrize("d,parents,offspring,gens", [(5, 32, 32, 8), (5, 1024, 3072, 3), (15, 32, 32, 8), (15, 1024, 3072, 3)])
def test_history_and_best_ever_against_a_twin(pkg, d, parents, offspring, gens):
    twin = odd_context(pkg, d, parents, offspring)
    twin.init_population(0)
    traj = []
    for _ in range(gens):
        twin.execute_generations(1)
        traj.append(twin.read_population())
    twin.close()
    es = odd_context(pkg, d, parents, offspring)
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


# ---- 6. whole runs: P = 64, N = 256 -------------------------------------------------------------------------------------------------
WAVES = {5: None, 15: [0, 7, 0, 1, 6]}
STALL = dict(target=None, stall=20, check_every=10)


def run_context(pkg, d, track=True, genes_off=False):
    """genes_off: the genes' range is [0, 0] - the same rows, every beta +0"""
    pmax = pmax_of(d)
    if genes_off:
        pmax = pmax[:d - len(gene_operators(GRAPHS[ODD[d][0]][0], ODD[d][1]))] + [0.0] * len(gene_operators(GRAPHS[ODD[d][0]][0], ODD[d][1]))
    name, mask = ODD[d]
    es = pkg.HipES(32, 32, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=8, param_max=pmax, seed=SEED, workgroup_size=32,
                   graph=pkg.capi.make_voice_graph(*GRAPHS[name]), feedback_genes=mask, waveforms=WAVES[d])
    if track:
        es.track()
    return es


def run_batch(pkg, d, slots, survivors=0):
    name, mask = ODD[d]
    b = pkg.HipBatch(slots, 32, 32, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=8, param_max=pmax_of(d), seed=SEED, workgroup_size=32,
                     graph=pkg.capi.make_voice_graph(*GRAPHS[name]), feedback_genes=mask, waveforms=WAVES[d])
    assert b.voice_feedback_genes() == mask and b.D == d
    b.track()
    b.set_survivors(survivors)
    return b


@pytest.mark.parametrize("d", WIDTHS)
def test_five_generations_stage_by_stage_equal_the_loop(pkg, table, d):
    name, mask = ODD[d]
    ops = GRAPHS[name][0]
    tg = targets(1, 256)[0]
    loop, staged, off = run_context(pkg, d, track=False), run_context(pkg, d, track=False), run_context(pkg, d, track=False, genes_off=True)
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
    assert not same_bits(want[2], other[2]), "the genes did not reach the generation loop"
    # the loop's last synthesis is the model's audio of the rows it evaluated
    v = want[0]
    model = graph_synth_genes(GRAPHS[name], codes_of(ops, None) if WAVES[d] is None else WAVES[d], [0.0] * ops, mask, v, [0.0] * d, pmax_of(d), 256, table)
    assert wrong_rows(synthesised(loop, v), model).size == 0
    for es in (loop, staged, off):
        es.close()


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


@pytest.mark.parametrize("d", WIDTHS)
def test_a_batch_and_a_two_slot_queue_with_a_carried_row_equal_sequential_contexts(pkg, d):
    tg = targets(3, 256)
    b = run_batch(pkg, d, 3)
    b.set_target_audio(tg)
    b.init_population(0)
    b.execute_generations(10)
    bv, bs, bf, bg = b.best_ever()
    es = run_context(pkg, d)
    for c in range(3):
        es.set_target_audio(tg[c])
        es.init_population(c)
        es.execute_generations(10)
        for what, a, w in zip(("values", "steps", "fitness"), b.read_population(c), es.read_population()):
            assert same_bits(a, w), (c, what)
        v, s, f, g = es.best_ever()
        assert same_bits(bv[c], v) and same_bits(bs[c], s) and same_bits(bf[c], f) and bg[c] == g, c
    es.close(); b.close()
    # the queue: two slots, one survivor, one carried row, segments of two chunks
    max_g, segment, rows = 60, 2, 1
    es = run_context(pkg, d)
    es.set_survivors(1)
    want = sequential_reference(pkg, es, tg, max_g, STALL, rows, segment)
    es.close()
    b = run_batch(pkg, d, 2, survivors=1)
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
        for field in ("best_ever_values", "best_ever_steps", "last_values"):
            assert np.all(got[k][field].view(np.uint32)[d:] == 0), (k, field)
    assert stats["slots"] == 2 and stats["chunk_generations"] == int(want["generations_run"].sum())


# ---- 7. rendering -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", WIDTHS)
def test_overlap_add_rendering_equals_the_accumulated_model_rows(pkg, O, table, d):
    """three rows that differ in beta: each is rendered with its own"""
    n, hop = 256, 128
    name, mask = ODD[d]
    ops = GRAPHS[name][0]
    v = R.unit_rows(3, d, 17)
    v[:, 2 * ops:] = np.array([[0.125], [0.5], [1.0]], np.float32)  # beta 0.25, 1 and 2 on every gene operator
    waves = codes_of(ops, None) if WAVES[d] is None else WAVES[d]
    rows = graph_synth_genes(GRAPHS[name], waves, [0.0] * ops, mask, v, [0.0] * d, pmax_of(d), n, table)
    same_beta = v.copy()
    same_beta[:, 2 * ops:] = 0.5
    assert not same_bits(rows[0], graph_synth_genes(GRAPHS[name], waves, [0.0] * ops, mask, same_beta, [0.0] * d, pmax_of(d), n, table)[0])
    es = run_context(pkg, d, track=False)
    for windowed in (True, False):
        got = es.render_overlap_add(v, hop, windowed=windowed)
        want = R.overlap_add(rows, hop, R.window32(O, n) if windowed else None)
        assert got.shape == want.shape == (2 * hop + n,) and same_bits(got, want), windowed
    es.close()
    assert np.abs(rows).max() > 0.01


# ---- 8. the search ------------------------------------------------------------------------------------------------------------------
def test_an_elitist_search_never_gets_worse_and_ends_on_an_index_within_bounds(pkg, table):
    """the feedback-sine target of DESIGN.md 4.15 (the additive pair with the second carrier's level 0 and an index of 1 on
    operator 0 at 430.66 Hz, bin 20 of N = 2048: the recipe of tools/graph_feedback_bench.py), searched by the 2-op graph
    with its carrier's index as a gene; one survivor, 50 generations, P = 64"""
    target = graph_synth_feedback(GRAPHS["additive"], [0, 0], [1.0, 0.0], np.ones((1, 4), np.float32), [0.0] * 4,
                                  [430.6640625, 1.0, 430.6640625, 0.0], 2048, table)[0]
    pmax = [3520.0, 8.0, 3520.0, 1.0]
    es = gene_es(pkg, "2op", 0b10, 32, 32, 11, None, pmax + [2.0])
    es.set_survivors(1)
    es.set_target_audio(target)
    es.init_population(0)
    es.track()
    best = []
    for _ in range(50):
        es.execute_generations(1)
        best.append(float(es.read_population()[2][0]))
    v, _, f, _ = es.best_ever()
    es.close()
    assert np.all(np.isfinite(best)) and np.all(np.diff(best) <= 0), best
    assert f == np.float32(best[-1])
    beta = float(effective_beta(np.float32(0.0) + v[4] * np.float32(2.0)))
    assert 0.0 <= beta <= 2.0, (beta, v)
