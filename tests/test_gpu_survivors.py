"""Elitist survival on the GPU (sots_set_survivors, sots_batch_set_survivors): rows 0..K-1 of the sorted half pass through
variation as bit copies, every other row is what it is with K = 0, and everything after variation is unchanged.

The reference in the stage tests is the CPU oracle composed by tests/_survivors_model.py (the oracle itself has no
survivors); in the batch and queue tests it is the sequential context with the same K, as in tests/test_gpu_batch.py and
tests/test_gpu_chunk_queue.py."""
import numpy as np
import pytest

from _survivors_model import PMAX, SEED, survivor_variation, targets

pytestmark = pytest.mark.gpu

SHIPPED = (16, 16, 32, 1, 11)   # parents, offspring, block, voice, log2 N: the reference's shipped sizes
CONFIG2 = (256, 768, 32, 0, 10)  # parameters.json


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def make(pkg, parents, offspring, block, kind, log2n, survivors=0, target=None, chunk=0):
    es = pkg.HipES(parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=block)
    if survivors:
        es.set_survivors(survivors)
    es.set_target_audio(targets(chunk + 1, 1 << log2n)[chunk] if target is None else target)
    es.init_population(chunk)
    return es


# ---- 1. stage parity against the oracle-composed generation ----------------------------------------------------------------
@pytest.mark.parametrize("parents,offspring,block,kind,log2n,k", [
    SHIPPED + (1,), SHIPPED + (16,),
    (64, 192, 32, 0, 10, 1), (64, 192, 32, 0, 10, 5), (64, 192, 32, 0, 10, 64),
    (30, 35, 5, 0, 9, 3), (30, 35, 5, 0, 9, 30)])  # block 5, 6 parent blocks: both slow paths of recombine_source
def test_stage_parity(pkg, O, parents, offspring, block, kind, log2n, k):
    """re-synchronised every generation as test_config2_trajectory_per_generation_parity does"""
    es = make(pkg, parents, offspring, block, kind, log2n, k)
    ref = O.OracleES(parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, recomb_block=block)
    for gen in range(3):
        v, s, f = es.read_population()
        ref.write_population(v, s, f)
        ev, es_ = O.recombine(v, s, parents, block)
        es.recombine()
        gv, gs, _ = es.read_population()
        assert same_bits(gv[:k], v[:k]) and same_bits(gs[:k], s[:k]), f"gen {gen}: recombine changed a survivor"
        assert same_bits(gv[k:], ev[k:]) and same_bits(gs[k:], es_[k:]), f"gen {gen}: recombine, rows >= K"
        es.mutate()
        gv, gs, _ = es.read_population()
        _, _, rv, rs = survivor_variation(ref, k, gen)
        assert same_bits(gv[:k], v[:k]) and same_bits(gs[:k], s[:k]), f"gen {gen}: mutate changed a survivor"
        assert same_bits(gv[k:], rv[k:]), f"gen {gen}: mutate, values of rows >= K"
        np.testing.assert_allclose(gs[k:], rs[k:], rtol=2e-6, atol=0)
        es.synthesise(); es.window(); es.fft(); es.fitness()
        gf = es.read_fitness()
        es.sort(); es.rotate()
        sv, ss, sf = es.read_population()
        perm = O.sort_perm(gf)
        assert same_bits(sf, gf[perm]) and same_bits(sv, gv[perm]) and same_bits(ss, gs[perm])
    assert es.generation == 3
    es.close()


# ---- 2. the fused loop equals the staged one, whichever kernel makes the individuals -----------------------------------------
# (voice, log2 N, parents, offspring, does the synthesis kernel make its individuals?) on the MI355X's 256 compute units:
FUSED_SHAPES = [
    (0, 10, 64, 192, True),         # k_synth_tp<2-op>: one individual per CU
    (1, 11, 16, 16, True),          # k_synth_tp<3-op>
    (2, 10, 32, 96, True),          # k_synth_tp<triple>
    (3, 12, 32, 96, True),          # k_synth_tp<4-op>
    (0, 10, 4096, 12288, True),     # k_synth<2-op, cut> with helper wavefronts: 64 per CU; selection kernels in the loop
    (3, 8, 4352, 13056, True),      # k_synth_ol<4-op>: 68 per CU
    (0, 9, 16416, 49152, True),     # k_synth<2-op, uncut> with helper wavefronts, two tiles; 513 parent blocks (no power of two)
    # the seven above all make their individuals inside the synthesis kernel; these two complete the list of sites:
    (2, 10, 512, 1536, False),      # triple voice at 8 per CU: no synthesis kernel makes individuals, k_recombine_mutate runs
    (0, 8, 32800, 98400, True),     # P > 131072: k_synth<2-op, uncut> loops over tiles, every lane makes its own individual
]


def fused_equals_staged(pkg, kind, log2n, parents, offspring, k, in_synth, mode=None):
    a = make(pkg, parents, offspring, 32, kind, log2n, k)
    b = make(pkg, parents, offspring, 32, kind, log2n, k)
    if mode is not None:
        a.set_sort_mode(mode); b.set_sort_mode(mode)
    a.timing_enable(True)
    a.execute_generations(3)
    for _ in range(3):
        b.execute_generation()
    _, launches = a.stage_time_ms(pkg.capi.STAGE_FUSED_VARIATION)
    rows = a.P
    if mode == pkg.capi.SORT_TOP_ONLY:  # rows behind the selected ones are unspecified in the fused loop
        block_rows = max(1, parents // 32) * 32
        rows = max(block_rows, parents)
    for x, y in zip(a.read_population(), b.read_population()):
        assert same_bits(x[:rows], y[:rows])
    a.close(); b.close()
    assert launches == (0 if in_synth else 3), launches
    return launches


@pytest.mark.parametrize("kind,log2n,parents,offspring,in_synth", FUSED_SHAPES)
@pytest.mark.parametrize("wide", [False, True])
def test_fused_equals_staged(pkg, kind, log2n, parents, offspring, in_synth, wide):
    """K = 1 and K = min(numParents, 70): 70 crosses a wavefront's 64 rows"""
    fused_equals_staged(pkg, kind, log2n, parents, offspring, min(parents, 70) if wide else 1, in_synth)


def test_fused_shapes_cover_both_variation_paths():
    assert {s[4] for s in FUSED_SHAPES} == {True, False}


def test_fused_equals_staged_under_the_other_sort_modes(pkg):
    fused_equals_staged(pkg, 3, 8, 4352, 13056, 70, True, pkg.capi.SORT_FULL)
    fused_equals_staged(pkg, 0, 10, 4096, 12288, 70, True, pkg.capi.SORT_TOP_ONLY)


# ---- 3. properties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SHIPPED, CONFIG2])
@pytest.mark.parametrize("plus", [False, True])
def test_properties_over_40_generations(pkg, shape, plus):
    """K = 1 and K = numParents (plus-selection), 40 generations of one call each, a history record every generation"""
    parents = shape[0]
    k = parents if plus else 1
    es = make(pkg, *shape, survivors=k)
    es.track(history_every=1, capacity=64)
    d = es.D
    best = []
    for gen in range(40):
        v0, s0, f0 = es.read_population()
        es.execute_generations(1)
        v1, s1, f1 = es.read_population()
        best.append(f1[0])
        if gen > 0:
            # a survivor is synthesised and evaluated again, at another row: the fitness must be the one it had.  (Rows are
            # found again by their bits; a survivor's offspring copy could share them only with equal fitness.)
            new = {}
            for i in range(es.P):
                new.setdefault(bits(v1[i]).tobytes() + bits(s1[i]).tobytes(), set()).add(int(bits(f1[i:i + 1])[0]))
            for i in range(k):
                got = new.get(bits(v0[i]).tobytes() + bits(s0[i]).tobytes())
                assert got is not None, f"gen {gen}: survivor {i} is not in the next population"
                assert int(bits(f0[i:i + 1])[0]) in got, f"gen {gen}: survivor {i} had {f0[i]!r}, re-evaluated to {sorted(got)}"
        bv, bs, bf, _ = es.best_ever()
        assert same_bits(bv, v1[0][:d]) and same_bits(bs, s1[0][:d]) and same_bits(bf, f1[0]), f"gen {gen}: best-ever is not row 0"
    assert all(b <= a for a, b in zip(best, best[1:])), best
    h = es.history()
    assert len(h) == 40 and same_bits(h["best_fitness"], h["best_ever_fitness"])
    assert same_bits(h["best_fitness"], np.array(best, np.float32))
    es.close()


@pytest.mark.parametrize("shape", [SHIPPED, CONFIG2])
def test_survivors_set_and_cleared_leave_the_library_untouched(pkg, shape):
    a, b = make(pkg, *shape), make(pkg, *shape)
    a.set_survivors(3)
    a.set_survivors(0)
    a.execute_generations(5); a.execute_generation()
    b.execute_generations(5); b.execute_generation()
    for x, y in zip(a.read_population(), b.read_population()):
        assert same_bits(x, y)
    a.close(); b.close()


# ---- 4. errors and state ------------------------------------------------------------------------------------------------------
def test_errors_and_state(pkg):
    es = make(pkg, *SHIPPED)
    assert es.survivors == 0
    es.set_survivors(16)
    es.set_survivors(4)
    with pytest.raises(pkg.SotsError) as e:
        es.set_survivors(17)
    assert e.value.code == -1 and "17" in str(e.value) and "numParents" in str(e.value)
    assert es.survivors == 4
    es.init_population(3)
    assert es.survivors == 4
    es.set_target_audio(targets(2, es.N)[1])
    assert es.survivors == 4
    v, s, f = es.read_population()
    es.write_population(v, s, f)
    assert es.survivors == 4
    es.close()
    b = pkg.HipBatch(2, 16, 16, synth_kind=1, audio_log2=11, param_max=PMAX[1], seed=SEED)
    with pytest.raises(pkg.SotsError) as e:
        b.set_survivors(17)
    assert e.value.code == -1 and "numParents" in str(e.value)
    b.set_survivors(16)
    b.close()


# ---- 5. chunks in flight ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parents,offspring,kind,log2n,k", [(16, 16, 1, 11, 1), (16, 16, 1, 11, 16), (256, 768, 0, 10, 1)])
def test_batch_equals_contexts(pkg, parents, offspring, kind, log2n, k):
    tg = targets(5, 1 << log2n)
    b = pkg.HipBatch(5, parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED)
    b.set_survivors(k)
    b.set_target_audio(tg)
    b.init_population(0)
    b.execute_generations(10)
    es = pkg.HipES(parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED)
    es.set_survivors(k)
    for c in range(5):
        es.set_target_audio(tg[c])
        es.init_population(c)
        es.execute_generations(10)
        for x, y in zip(b.read_population(c), es.read_population()):
            assert same_bits(x, y), f"chunk {c}"
    b.close(); es.close()


# ---- 6. chunk queue -----------------------------------------------------------------------------------------------------------
def test_queue_equals_sequential_contexts(pkg):
    """7 chunks through 3 slots under a stall rule: every result, and the kept population, is that of a sequential tracked
    context with the same K (a refilled slot's first variation carries the initialised rows 0..K-1, as a fresh context's)"""
    parents, offspring, kind, log2n, k, chunks, keep = 16, 16, 1, 11, 1, 7, 4
    rule = dict(target=None, stall=20, check_every=5)
    tg = targets(chunks, 1 << log2n)
    d = pkg.capi.SYNTH_DIMS[kind]
    es = pkg.HipES(parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED)
    es.track()
    es.set_survivors(k)
    want, pops = np.zeros(chunks, pkg.capi.CHUNK_RESULT_DTYPE), []
    for c in range(chunks):
        es.set_target_audio(tg[c])
        es.init_population(c)
        run = es.execute_until(60, **rule)
        v, s, f, g = es.best_ever()
        pop = es.read_population()
        r = want[c]
        r["generations_run"], r["best_ever_generation"], r["best_ever_fitness"], r["last_fitness"] = run, g, f, pop[2][0]
        r["best_ever_values"][:d], r["best_ever_steps"][:d], r["last_values"][:d] = v, s, pop[0][0]
        pops.append(pop)
    es.close()
    b = pkg.HipBatch(3, parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED)
    b.track()
    b.set_survivors(k)
    b.queue_targets_audio(tg)
    got, stats = b.queue_run(0, 60, keep=keep, **rule)
    kept = b.queue_kept_population()
    b.close()
    print("generations run:", want["generations_run"].tolist(), stats)
    assert len(got) == chunks
    for c in range(chunks):
        for name in ("generations_run", "best_ever_generation"):
            assert got[c][name] == want[c][name], (c, name, got[c][name], want[c][name])
        for name in ("best_ever_fitness", "last_fitness", "best_ever_values", "best_ever_steps", "last_values"):
            assert same_bits(got[c][name], want[c][name]), (c, name, got[c][name], want[c][name])
    for x, y in zip(kept, pops[keep]):
        assert same_bits(x, y)


# ---- 7. island group ----------------------------------------------------------------------------------------------------------
def test_group_islands_keep_their_best(pkg):
    """two islands on device 0, 2 elites exchanged every generation, K = 2 set through island(i)"""
    g = pkg.HipGroup([0, 0], 2, 64, 192, pkg.capi.SYNTH_2OP, 10, None, PMAX[0], seed=SEED, migration_interval=1)
    for i in range(2):
        g.island(i).set_survivors(2)
    g.set_target_audio(targets(1, 1024)[0])
    g.init_population(0)
    best = [[], []]
    for _ in range(6):
        g.execute_generations(1)
        g.synchronize()
        for i in range(2):
            assert g.island(i).survivors == 2
            best[i].append(g.island(i).read_population()[2][0])
    g.close()
    for i in range(2):
        assert all(b <= a for a, b in zip(best[i], best[i][1:])), (i, best[i])


# ---- 8. quality ---------------------------------------------------------------------------------------------------------------
def test_one_survivor_beats_the_best_ever_record_of_the_plain_run(pkg):
    """The 8 noisy shipped chunks in one tracked batch, 200 generations.  The GPU's trajectories leave the oracle's at the
    first near-tie, so the conditions are orderings, not the oracle's values: on the CPU model every chunk's final row 0
    with K = 1 lies at least 87x below that with K = 0 (chunk 6), and the mean final row 0 with K = 1 is 0.13 against a
    mean best-ever fitness of 38.8 with K = 0."""
    tg = targets(8, 2048)
    last, ever = {}, {}
    for k in (0, 1):
        b = pkg.HipBatch(8, 16, 16, synth_kind=1, audio_log2=11, param_max=PMAX[1], seed=SEED)
        b.track()
        b.set_survivors(k)
        b.set_target_audio(tg)
        b.init_population(0)
        b.execute_generations(200)
        last[k] = b.read_best()[1].astype(np.float64)
        ever[k] = b.best_ever()[2].astype(np.float64)
        b.close()
    print("final row 0, K = 0:", last[0], "\nfinal row 0, K = 1:", last[1], "\nbest ever, K = 0:", ever[0])
    assert np.all(last[1] <= last[0])
    assert last[1].mean() <= ever[0].mean()
    assert np.array_equal(last[1], ever[1])
