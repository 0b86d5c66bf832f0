"""Per-bin weights of the spectral objective on the GPU (sots_set_objective_weights): F = sum_k w_k e_k^2
against the fp64 model (tests/_weights_model.py), fused against staged, the two exact properties (weight 1: the unweighted
bits; weight 0: the bin is not looked at), the state rules, the selection plans, and the batch, the queue, the group and the
elitist run under weights.

Tolerance of a device fitness against the model, per row (derived from what the project documents, not picked):
    |F_dev - F_model| <= sum_k w_k (2 |e_k| d_k + d_k^2) + 1e-4 F_model
with d_k = delta under MAGNITUDE and delta / (m_k + eps) + LAMBDA under LOG_MAGNITUDE; delta = 3e-6 max_k m_k over all
bins, the masked ones included (the transform's error does not know the weights), LAMBDA = 2.5e-6 as in
tests/test_gpu_objective.py.

The weight vector is _weights_model.fixed_weights: uniform in [0, 2] with a fixed seed, zeros on bins N/8 .. N/4, exact
ones on the N/16 bins behind them.  The shapes are test_gpu_objective.py's."""
import os
import sys

import numpy as np
import pytest

from _objective_model import magnitudes
from _weights_model import fixed_weights, tolerance, weighted_distance

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from track_overhead import targets  # noqa: E402

LAMBDA = 2.5e-6
FLOORS = (1e-2, 1e-4)
OBJECTIVES = (None, 1e-4)  # None: MAGNITUDE; a number: LOG_MAGNITUDE with that floor
PMAX = {0: [3520.0, 8.0, 3520.0, 1.0],
        1: [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0]}
TARGET = {0: [1450.0 / 3520.0, 3.0 / 8.0, 200.0 / 3520.0, 1.0],
          1: [3078 / 3520.0, 2.0 / 8.0, 3015 / 3520.0, 1.5 / 8.0, 3141 / 3520.0, 1.0 / 8.0]}
SEED = 0x5EED0001

# (voice, log2 N, P): the smallest shapes that reach each kernel family of launch_fft_fitness; parents = P / 4
SHAPES = [
    (0, 8, 64),        # k_fft_x<8>
    (0, 9, 64),        # k_fft<9>
    (0, 10, 64),       # k_fft<10>, one wavefront
    (1, 10, 64),       # ... the 3-op voice
    (0, 10, 3072),     # k_fft<10>, the wide form
    (0, 11, 64),       # k_fft_x<11>, four wavefronts
    (0, 12, 4096),     # k_fft_x<12>, full workgroups: ceil(P / 16) >= 256 CUs
    (0, 13, 32),       # k_fft_x<13>
    (0, 14, 32),       # k_fft_big
]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def set_obj(pkg, es, eps):
    if eps is None:
        es.set_objective(pkg.capi.OBJECTIVE_MAGNITUDE)
    else:
        es.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, eps)


def make(pkg, O, kind, log2n, p, eps=None, weights=None, target=True, **kw):
    es = pkg.HipES(p // 4, p - p // 4, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=32, **kw)
    if eps is not None:
        set_obj(pkg, es, eps)
    if weights is not None:
        es.set_objective_weights(weights)
    if target:
        es.set_target_audio(target_audio(O, kind, es.N))
    return es


_TARGETS = {}


def target_audio(O, kind, n):
    if (kind, n) not in _TARGETS:
        _TARGETS[kind, n] = O.synth(kind, TARGET[kind], [0.0] * len(TARGET[kind]), PMAX[kind], n)
    return _TARGETS[kind, n]


def staged_fitness(es):
    es.init_population(0)
    es.synthesise(); es.window(); es.fft(); es.fitness()
    return es.read_fitness()


# ---- 1. staged fitness() against the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n,p", SHAPES)
def test_staged_fitness_against_the_model(pkg, O, kind, log2n, p):
    w = fixed_weights(1 << log2n)
    es = make(pkg, O, kind, log2n, p, weights=w)
    es.init_population(0)
    es.synthesise()
    audio = es.read_audio()
    t = es.read_target()
    np.testing.assert_allclose(t, O.spectrum(target_audio(O, kind, es.N)), rtol=1e-6, atol=1e-9)  # raw magnitudes under weights
    m = magnitudes(O, audio)
    es.window(); es.fft()
    for eps in (None,) + FLOORS:
        set_obj(pkg, es, eps)
        es.fitness()
        f = es.read_fitness().astype(np.float64)
        want = weighted_distance(m, t, w, eps)
        tol = tolerance(m, t, w, eps, LAMBDA)
        err = np.abs(f - want)
        worst = int(np.argmax(err / tol))
        print(f"voice {kind} N {es.N} P {p} objective {'magnitude' if eps is None else 'log, eps %g' % eps}: F {want.min():.4g} .. {want.max():.4g}; "
              f"worst row {worst}: |dF| {err[worst]:.3g} of bound {tol[worst]:.3g} (|dF| / bound {err[worst] / tol[worst]:.3g})")
        assert np.all(np.isfinite(f))
        assert np.all(err <= tol), (eps, worst, f[worst], want[worst], tol[worst])
    es.close()


# ---- 2. fused equals staged, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", OBJECTIVES)
@pytest.mark.parametrize("kind,log2n,p", SHAPES)
def test_fused_generation_equals_staged(pkg, O, kind, log2n, p, eps):
    w = fixed_weights(1 << log2n)
    a, b = make(pkg, O, kind, log2n, p, eps, w), make(pkg, O, kind, log2n, p, eps, w)
    for e in (a, b):
        e.init_population(0)
    a.execute_generations(1)
    b.execute_generation()
    for name, x, y in zip(("values", "steps", "fitness"), a.read_population(), b.read_population()):
        assert same_bits(x, y), name
    assert np.all(np.isfinite(a.read_fitness())) and a.read_fitness()[0] > 0.0
    a.close(); b.close()


# ---- 3. all-ones weights are no weights, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("eps", OBJECTIVES)
@pytest.mark.parametrize("kind,log2n,p", SHAPES)
def test_all_ones_weights_equal_no_weights(pkg, O, kind, log2n, p, eps):
    plain = make(pkg, O, kind, log2n, p, eps)
    ones = make(pkg, O, kind, log2n, p, eps, np.ones((1 << log2n) // 2, np.float32))
    assert same_bits(staged_fitness(plain), staged_fitness(ones))
    for e in (plain, ones):
        e.init_population(0)
        e.execute_generations(3)
    for name, x, y in zip(("values", "steps", "fitness"), plain.read_population(), ones.read_population()):
        assert same_bits(x, y), name
    plain.close(); ones.close()


# ---- 4. a zero weight: the bin is not looked at -------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", OBJECTIVES)
@pytest.mark.parametrize("kind,log2n,p", [(0, 10, 64), (0, 11, 64), (0, 14, 32)])
def test_zero_weight_bins_are_not_looked_at(pkg, O, kind, log2n, p, eps):
    """two targets that differ only where the weight is 0: the same fitness bits, staged and after a fused generation"""
    n = 1 << log2n
    w = fixed_weights(n)
    zero = np.flatnonzero(w == 0.0)
    assert zero.size >= n // 8
    t1 = np.asarray(O.spectrum(target_audio(O, kind, n)), np.float32)[: n // 2].copy()
    t2 = t1.copy()
    t2[zero] = t1[zero] * 3.0 + 0.25
    got = []
    for t in (t1, t2):
        es = make(pkg, O, kind, log2n, p, eps, w, target=False)
        es.set_target_spectrum(t)
        f = staged_fitness(es)
        es.init_population(0)
        es.execute_generations(1)
        got.append((f, es.read_fitness()))
        es.close()
    assert same_bits(got[0][0], got[1][0]) and same_bits(got[0][1], got[1][1])
    assert np.all(np.isfinite(got[0][0])) and np.all(got[0][0] > 0.0)
    # ... and they do count without the weights
    es = make(pkg, O, kind, log2n, p, eps, target=False)
    es.set_target_spectrum(t1)
    f1 = staged_fitness(es)
    es.set_target_spectrum(t2)
    f2 = staged_fitness(es)
    es.close()
    assert not same_bits(f1, f2)


# ---- 5. state -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", OBJECTIVES)
@pytest.mark.parametrize("log2n", [10, 11])
def test_weights_before_or_after_the_target_and_the_objective(pkg, O, log2n, eps):
    """N = 2048 too: there the fused kernel reads the table image"""
    w = fixed_weights(1 << log2n)
    first = make(pkg, O, 0, log2n, 64, None, w, target=False)       # weights, objective, target
    if eps is not None:
        set_obj(pkg, first, eps)
    first.set_target_audio(target_audio(O, 0, first.N))
    last = make(pkg, O, 0, log2n, 64, eps)                          # objective, target, weights
    last.set_objective_weights(w)
    middle = make(pkg, O, 0, log2n, 64, target=True)                # target, weights, objective
    middle.set_objective_weights(w)
    set_obj(pkg, middle, eps)
    f = staged_fitness(first)
    assert same_bits(f, staged_fitness(last)) and same_bits(f, staged_fitness(middle))
    for e in (first, last, middle):
        e.init_population(0)
        e.execute_generations(2)
    for other in (last, middle):
        for x, y in zip(first.read_population(), other.read_population()):
            assert same_bits(x, y)
    first.close(); last.close(); middle.close()


@pytest.mark.parametrize("eps", OBJECTIVES)
@pytest.mark.parametrize("log2n", [10, 11])
def test_removing_the_weights_gives_the_bits_of_a_context_that_never_had_them(pkg, O, log2n, eps):
    plain = make(pkg, O, 0, log2n, 64, eps)
    back = make(pkg, O, 0, log2n, 64, eps)
    f_plain = staged_fitness(plain)
    back.set_objective_weights(fixed_weights(1 << log2n))
    assert not same_bits(staged_fitness(back), f_plain)
    back.set_objective_weights(None)
    assert back.get_objective_weights() is None
    assert same_bits(staged_fitness(back), f_plain)
    for e in (plain, back):
        e.init_population(0)
        e.execute_generations(2)
    for x, y in zip(plain.read_population(), back.read_population()):
        assert same_bits(x, y)
    plain.close(); back.close()


def test_get_round_trips_and_bad_weights_are_refused(pkg, O):
    es = make(pkg, O, 0, 10, 64)
    assert es.get_objective_weights() is None
    w = fixed_weights(1024)
    es.set_objective_weights(w)
    assert same_bits(es.get_objective_weights(), w)
    f = staged_fitness(es)
    neg, nan, inf = w.copy(), w.copy(), w.copy()
    neg[17], nan[400], inf[511] = -1e-3, np.nan, np.inf
    for bad, text in ((w[:511], "need 512 bins, got 511"), (np.concatenate([w, w]), "need 512 bins, got 1024"),
                      (neg, "weight 17 is -0.001"), (nan, "weight 400 is nan"), (inf, "weight 511 is inf"),
                      (np.zeros(512, np.float32), "all zero")):
        with pytest.raises(pkg.capi.SotsError) as err:
            es.set_objective_weights(bad)
        assert text in str(err.value), (text, str(err.value))
        assert same_bits(es.get_objective_weights(), w)             # the old table stays
        assert same_bits(staged_fitness(es), f)
    b = pkg.HipBatch(2, 16, 16, synth_kind=0, audio_log2=10, param_max=PMAX[0], seed=SEED, workgroup_size=32)
    for bad, text in ((w[:100], "need 512 bins, got 100"), (neg, "weight 17 is"), (np.zeros(512, np.float32), "all zero")):
        with pytest.raises(pkg.capi.SotsError) as err:
            b.set_objective_weights(bad)
        assert text in str(err.value)
    b.set_objective_weights(w)
    b.set_objective_weights(None)
    b.close()
    es.close()


def test_setting_weights_clears_the_best_ever_record(pkg, O):
    es = make(pkg, O, 0, 10, 64)
    es.track()
    es.init_population(0)
    es.execute_generations(3)
    _, _, f, g = es.best_ever()
    assert np.isfinite(f) and 1 <= g <= 3
    es.set_objective_weights(fixed_weights(1024))
    _, _, f, g = es.best_ever()
    assert np.isinf(f) and g == 0
    es.execute_generations(2)
    _, _, f, g = es.best_ever()
    assert np.isfinite(f) and 4 <= g <= 5
    es.set_objective_weights(None)                                  # removing them is a new start too
    assert np.isinf(es.best_ever()[2])
    es.close()


# ---- 6. the selection plans ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", OBJECTIVES)
def test_select_plans_agree_under_weights(pkg, O, eps):
    """P = 4096 + 12288, N = 1024: from generation 2 AUTO runs the list mode - the weighted instantiation of the bucketing
    kernel - beside TILES and the streaming SPLITTERS; all three place the same rows"""
    pops = []
    for plan in (pkg.capi.SELECT_AUTO, pkg.capi.SELECT_TILES, pkg.capi.SELECT_SPLITTERS):
        es = pkg.HipES(4096, 12288, synth_kind=0, audio_log2=10, param_max=PMAX[0], seed=SEED, workgroup_size=32)
        set_obj(pkg, es, eps)
        es.set_objective_weights(fixed_weights(1024))
        es.set_target_audio(target_audio(O, 0, 1024))
        es.set_select_plan(plan)
        es.init_population(0)
        es.execute_generations(6)
        pops.append(es.read_population())
        es.close()
    for other in pops[1:]:
        for name, x, y in zip(("values", "steps", "fitness"), pops[0], other):
            assert same_bits(x, y), name
    f = pops[0][2]
    assert np.all(np.diff(f[:4096]) >= 0) and np.all(np.isfinite(f))


# ---- 7. carried by the rest ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", OBJECTIVES)
@pytest.mark.parametrize("kind,log2n,parents,offspring,chunks", [(1, 11, 8, 24, 8), (0, 10, 256, 768, 4)])
def test_batch_equals_sequential_contexts(pkg, kind, log2n, parents, offspring, chunks, eps):
    kw = dict(synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=32)
    w = fixed_weights(1 << log2n)
    tg = targets(chunks, 1 << log2n)
    b = pkg.HipBatch(chunks, parents, offspring, **kw)
    b.set_target_audio(tg)          # the targets first, objective and weights after them
    set_obj(pkg, b, eps)
    b.set_objective_weights(w)
    b.track()
    b.init_population(0)
    b.execute_generations(20)
    b.synchronize()
    ever = b.best_ever()
    es = pkg.HipES(parents, offspring, **kw)
    set_obj(pkg, es, eps)
    es.set_objective_weights(w)
    es.track()
    for c in range(chunks):
        es.set_target_audio(tg[c])
        es.init_population(c)
        es.execute_generations(20)
        for name, x, y in zip(("values", "steps", "fitness"), b.read_population(c), es.read_population()):
            assert same_bits(x, y), (c, name)
        v, s, f, g = es.best_ever()
        assert same_bits(ever[0][c], v) and same_bits(ever[1][c], s) and same_bits(ever[2][c], f) and ever[3][c] == g, c
    es.close(); b.close()


@pytest.mark.parametrize("eps", OBJECTIVES)
@pytest.mark.parametrize("shape", [(1, 11, 16, 16), (0, 10, 32, 32)])
def test_queue_equals_sequential_tracked_contexts(pkg, shape, eps):
    """6 chunks through 4 slots under a stall rule (the shapes of tests/test_gpu_chunk_queue.py)"""
    kind, log2n, parents, offspring = shape
    kw = dict(synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=32)
    rule = dict(target=None, stall=50, check_every=25)
    w = fixed_weights(1 << log2n)
    tg = targets(6, 1 << log2n)
    b = pkg.HipBatch(4, parents, offspring, **kw)
    b.track()
    b.set_objective_weights(w)      # the weights first, the stored targets and the objective after them
    b.queue_targets_audio(tg)
    set_obj(pkg, b, eps)
    got, stats = b.queue_run(0, 400, **rule)
    b.close()
    d = pkg.capi.SYNTH_DIMS[kind]
    es = pkg.HipES(parents, offspring, **kw)
    set_obj(pkg, es, eps)
    es.set_objective_weights(w)
    es.track()
    runs = []
    for k in range(6):
        es.set_target_audio(tg[k])
        es.init_population(k)
        run = es.execute_until(400, **rule)
        v, s, f, g = es.best_ever()
        pop = es.read_population()
        r = got[k]
        assert (r["generations_run"], r["best_ever_generation"]) == (run, g), k
        assert same_bits(r["best_ever_fitness"], f) and same_bits(r["last_fitness"], pop[2][0]), k
        assert same_bits(r["best_ever_values"][:d], v) and same_bits(r["best_ever_steps"][:d], s) and same_bits(r["last_values"][:d], pop[0][0]), k
        runs.append(run)
    es.close()
    print(f"shape {shape}: generations_run {runs}, global {stats['global_generations']}")
    assert stats["slots"] == 4 and stats["chunk_generations"] == sum(runs)


def test_group_sets_every_island(pkg, O):
    kw = dict(synth_kind=0, audio_log2=10, param_max=PMAX[0], seed=SEED, workgroup_size=32)
    w = fixed_weights(1024)
    g = pkg.HipGroup([0, 0], 4, 64, 192, migration_interval=1000, **kw)
    g.set_objective_weights(w)
    g.set_target_audio(target_audio(O, 0, 1024))
    g.init_population(0)
    g.execute_generations(1)
    g.synchronize()
    for i in range(2):
        isl = g.island(i)
        assert same_bits(isl.get_objective_weights(), w)
        es = pkg.HipES(64, 192, gid_base=i * 256, **kw)
        es.set_objective_weights(w)
        es.set_target_audio(target_audio(O, 0, 1024))
        es.init_population(0)
        es.execute_generations(1)
        for name, x, y in zip(("values", "steps", "fitness"), isl.read_population(), es.read_population()):
            assert same_bits(x, y), (i, name)
        es.close()
    with pytest.raises(pkg.capi.SotsError) as err:
        g.set_objective_weights(np.zeros(512, np.float32))
    assert "island 0" in str(err.value) and "all zero" in str(err.value)
    g.close()


@pytest.mark.parametrize("eps", OBJECTIVES)
def test_elitist_run_never_gets_worse(pkg, O, eps):
    es = make(pkg, O, 0, 10, 1024, eps, fixed_weights(1024))
    es.set_survivors(1)
    es.init_population(0)
    best = []
    for _ in range(30):
        es.execute_generations(1)
        best.append(float(es.read_fitness()[0]))
    es.close()
    print(f"row 0 under weights: generation 1 {best[0]:.6g}, generation 30 {best[-1]:.6g}")
    assert all(y <= x for x, y in zip(best, best[1:]))
    assert best[-1] < best[0]
