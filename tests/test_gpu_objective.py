"""The selectable spectral objective on the GPU (sots_set_objective): the log-magnitude distance with a floor
against the fp64 model (tests/_objective_model.py), fused against staged, its semantics, and the batch, the queue, the
group and the elitist run under it.

Tolerance of a device fitness against the model, per row (derived, not picked):
    |F_dev - F_model| <= sum_k (2 |e_k| d_k + d_k^2) + 1e-4 F_model,   d_k = delta / (m_k + eps) + LAMBDA
delta = 3e-6 max_k m_k is the documented per-bin error of the fp32 transform, 1e-4 the project's relative fitness
tolerance, and LAMBDA bounds the absolute error of the device's ln(m + eps) against fp64 log for arguments in [eps, 2].
LAMBDA = 2.5e-6 is twice the largest error tools/ubench/ln_map_error measured on the MI355X for the floors used here
(1.214e-6 at eps = 1e-4, 6.3e-7 at 1e-2; every 23rd fp32 magnitude from the smallest normal number to 2 - eps, and 0,
against libm's fp64 log of the exact sum), rounded up.
The floors are 1e-2 and 1e-4: below that the bound grows useless (3.6 % of F at 1e-5)."""
import os
import sys

import numpy as np
import pytest

from _objective_model import log_distance, magnitudes, tolerance

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from track_overhead import targets  # noqa: E402

LAMBDA = 2.5e-6
FLOORS = (1e-2, 1e-4)
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


def make(pkg, O, kind, log2n, p, eps=None, target=True, **kw):
    es = pkg.HipES(p // 4, p - p // 4, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=32, **kw)
    if eps is not None:
        es.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, eps)
    if target:
        es.set_target_audio(target_audio(O, kind, es.N))
    return es


_TARGETS = {}


def target_audio(O, kind, n):
    if (kind, n) not in _TARGETS:
        _TARGETS[kind, n] = O.synth(kind, TARGET[kind], [0.0] * len(TARGET[kind]), PMAX[kind], n)
    return _TARGETS[kind, n]


# ---- 1. staged fitness() against the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n,p", SHAPES)
def test_staged_fitness_against_the_model(pkg, O, kind, log2n, p):
    es = make(pkg, O, kind, log2n, p, FLOORS[0])
    es.init_population(0)
    v, s, _ = es.read_population()
    v[5] = TARGET[kind]  # the self-match row
    es.write_population(v, s, None)
    es.synthesise()
    audio = es.read_audio()
    t = es.read_target()
    np.testing.assert_allclose(t, O.spectrum(target_audio(O, kind, es.N)), rtol=1e-6, atol=1e-9)  # raw magnitudes under LOG
    m = magnitudes(O, audio)
    es.window(); es.fft()
    for eps in FLOORS:
        es.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, eps)
        es.fitness()
        f = es.read_fitness().astype(np.float64)
        want = log_distance(m, t, eps)
        tol = tolerance(m, t, eps, LAMBDA)
        err = np.abs(f - want)
        worst = int(np.argmax(err / tol))
        print(f"voice {kind} N {es.N} P {p} eps {eps}: F {want.min():.4g} .. {want.max():.4g}; worst row {worst}: |dF| {err[worst]:.3g} of bound "
              f"{tol[worst]:.3g} (bound / F {tol[worst] / max(want[worst], 1e-300):.2g}); largest bound / F over the other rows "
              f"{np.max(np.delete(tol / np.maximum(want, 1e-300), 5)):.2g}")
        assert np.all(np.isfinite(f))
        assert np.all(err <= tol), (eps, worst, f[worst], want[worst], tol[worst])
    es.close()


# ---- 2. fused equals staged, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n,p", SHAPES)
def test_fused_generation_equals_staged(pkg, O, kind, log2n, p):
    a, b = make(pkg, O, kind, log2n, p, FLOORS[1]), make(pkg, O, kind, log2n, p, FLOORS[1])
    for e in (a, b):
        e.init_population(0)
    a.execute_generations(1)
    b.execute_generation()
    for name, x, y in zip(("values", "steps", "fitness"), a.read_population(), b.read_population()):
        assert same_bits(x, y), name
    assert np.all(np.isfinite(a.read_fitness())) and a.read_fitness()[0] > 0.0
    a.close(); b.close()


def test_select_plans_agree_under_the_log_objective(pkg, O):
    """P = 4096 + 12288, N = 1024: from generation 2 AUTO runs the list mode - the log instantiation of the bucketing
    kernel - beside TILES and the streaming SPLITTERS; all three place the same rows"""
    pops = []
    for plan in (pkg.capi.SELECT_AUTO, pkg.capi.SELECT_TILES, pkg.capi.SELECT_SPLITTERS):
        es = pkg.HipES(4096, 12288, synth_kind=0, audio_log2=10, param_max=PMAX[0], seed=SEED, workgroup_size=32)
        es.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, FLOORS[1])
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


# ---- 3. semantics -------------------------------------------------------------------------------------------------------------
def staged_fitness(es):
    es.init_population(0)
    es.synthesise(); es.window(); es.fft(); es.fitness()
    return es.read_fitness()


@pytest.mark.parametrize("log2n", [10, 11])
def test_objective_before_or_after_the_target(pkg, O, log2n):
    """N = 2048 too: there the fused kernel reads the table image, which both orders must rebuild"""
    first = make(pkg, O, 0, log2n, 64, FLOORS[1])
    after = make(pkg, O, 0, log2n, 64)
    after.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, FLOORS[1])
    assert same_bits(staged_fitness(first), staged_fitness(after))
    for e in (first, after):
        e.init_population(0)
        e.execute_generations(2)
    for x, y in zip(first.read_population(), after.read_population()):
        assert same_bits(x, y)
    first.close(); after.close()


@pytest.mark.parametrize("log2n", [10, 11])
def test_switching_back_gives_the_bits_of_a_context_that_never_switched(pkg, O, log2n):
    plain = make(pkg, O, 0, log2n, 64)
    back = make(pkg, O, 0, log2n, 64)
    f_mag = staged_fitness(plain)
    back.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, FLOORS[0])
    f_log = staged_fitness(back)
    assert not same_bits(f_log, f_mag)
    back.set_objective(pkg.capi.OBJECTIVE_MAGNITUDE)
    assert back.objective == (pkg.capi.OBJECTIVE_MAGNITUDE, 0.0)
    assert same_bits(staged_fitness(back), f_mag)
    for e in (plain, back):
        e.init_population(0)
        e.execute_generations(2)
    for x, y in zip(plain.read_population(), back.read_population()):
        assert same_bits(x, y)
    plain.close(); back.close()


def test_get_objective_round_trips_and_bad_settings_are_refused(pkg, O):
    es = make(pkg, O, 0, 10, 64)
    assert es.objective == (pkg.capi.OBJECTIVE_MAGNITUDE, 0.0)
    es.set_objective(pkg.capi.OBJECTIVE_MAGNITUDE, 0.25)  # the floor is ignored and reported as 0
    assert es.objective == (pkg.capi.OBJECTIVE_MAGNITUDE, 0.0)
    for eps in (1e-30, 1e-4, 1.0):
        es.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, eps)
        assert es.objective == (pkg.capi.OBJECTIVE_LOG_MAGNITUDE, float(np.float32(eps)))
    for obj, eps, text in ((2, 1e-3, "unknown objective 2"), (7, 0.0, "unknown objective 7"),
                           (1, 0.0, "floor 0 outside"), (1, -1e-3, "outside 1e-30 .. 1"), (1, float("nan"), "outside 1e-30 .. 1"),
                           (1, float("inf"), "outside 1e-30 .. 1"), (1, 1.5, "floor 1.5 outside"), (1, 1e-31, "outside 1e-30 .. 1")):
        with pytest.raises(pkg.capi.SotsError) as err:
            es.set_objective(obj, eps)
        assert text in str(err.value), (obj, eps, str(err.value))
        assert es.objective == (pkg.capi.OBJECTIVE_LOG_MAGNITUDE, 1.0)  # the old setting stays
    b = pkg.HipBatch(2, 16, 16, synth_kind=0, audio_log2=10, param_max=PMAX[0], seed=SEED, workgroup_size=32)
    with pytest.raises(pkg.capi.SotsError) as err:
        b.set_objective(1, 2.0)
    assert "floor 2 outside" in str(err.value)
    with pytest.raises(pkg.capi.SotsError):
        b.set_objective(3, 1e-3)
    b.close()
    es.close()


def test_set_objective_clears_the_best_ever_record(pkg, O):
    es = make(pkg, O, 0, 10, 64)
    es.track()
    es.init_population(0)
    es.execute_generations(3)
    _, _, f, g = es.best_ever()
    assert np.isfinite(f) and 1 <= g <= 3
    es.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, FLOORS[0])
    _, _, f, g = es.best_ever()
    assert np.isinf(f) and g == 0
    es.execute_generations(2)
    _, _, f, g = es.best_ever()
    assert np.isfinite(f) and 4 <= g <= 5
    es.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, FLOORS[0])  # the same setting again: still a new start
    assert np.isinf(es.best_ever()[2])
    es.close()


def test_a_spectrum_with_the_targets_magnitudes_has_fitness_exactly_zero(pkg, O):
    """N = 1024: the window factor is exactly 1 and 1/N a power of two, so a spectrum of powers of two r_k has the
    magnitudes r_k / N to the bit - the magnitude objective's exact 0 below confirms it - and the target table, made by
    the routine the epilogue applies to the candidate, cancels every bin exactly"""
    es = make(pkg, O, 0, 10, 64, target=False)
    n = es.N
    k = np.arange(n // 2)
    r = np.where(k % 7 == 3, 0.0, 2.0 ** -(k % 13).astype(np.float64)).astype(np.float32)
    spec = np.zeros((es.P, n + 8), np.float32)
    spec[:, 0:n:2] = r[None, :]                                     # real parts of bins 0 .. N/2-1
    spec[3] = 0.0
    spec[3, 0:n:2] = 0.5 * r                                        # a row that is NOT the target
    es.set_target_spectrum(r / np.float32(n))
    es.write_spectrum(spec)
    es.fitness()
    f = es.read_fitness()
    assert np.all(np.delete(f, 3) == 0.0) and f[3] > 0.0
    for eps in FLOORS + (1e-30, 1.0):
        es.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, eps)
        es.fitness()
        f = es.read_fitness()
        assert np.all(np.delete(f, 3) == 0.0), (eps, f)
        half, full = 0.5 * r.astype(np.float64) / n, r.astype(np.float64) / n
        want = log_distance(half, full, eps)
        assert abs(f[3] - want) <= tolerance(half, full, eps, LAMBDA), (eps, f[3], want)
    es.close()


def test_nan_rows_get_nan_fitness_and_sort_last(pkg, O):
    es = make(pkg, O, 0, 10, 64, FLOORS[0])
    es.init_population(0)
    es.synthesise()
    a = es.read_audio()
    a[7] = np.nan
    es.write_audio(a)
    es.window(); es.fft(); es.fitness()
    f = es.read_fitness()
    assert np.isnan(f[7]) and np.all(np.isfinite(np.delete(f, 7)))
    es.sort(); es.rotate()
    f = es.read_fitness()
    assert np.isnan(f[-1]) and np.all(np.diff(f[:-1]) >= 0)
    es.close()


# ---- 4. batch against sequential contexts ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n,parents,offspring,chunks", [(1, 11, 16, 16, 4), (0, 10, 256, 768, 4)])
def test_batch_equals_sequential_contexts(pkg, kind, log2n, parents, offspring, chunks):
    kw = dict(synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=32)
    tg = targets(chunks, 1 << log2n)
    b = pkg.HipBatch(chunks, parents, offspring, **kw)
    b.set_target_audio(tg)          # the targets first, the objective after them: the image is rebuilt
    b.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, FLOORS[1])
    b.track()
    b.init_population(0)
    b.execute_generations(20)
    b.synchronize()
    ever = b.best_ever()
    es = pkg.HipES(parents, offspring, **kw)
    es.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, FLOORS[1])
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


# ---- 5. queue against sequential tracked contexts -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 11, 16, 16), (0, 10, 32, 32)])
def test_queue_equals_sequential_tracked_contexts(pkg, shape):
    """6 chunks through 4 slots under a stall rule (the shapes of tests/test_gpu_chunk_queue.py: k_fft_x's table, which the
    turnover rewrites, and the plain bins)"""
    kind, log2n, parents, offspring = shape
    kw = dict(synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=32)
    rule = dict(target=None, stall=50, check_every=25)
    tg = targets(6, 1 << log2n)
    b = pkg.HipBatch(4, parents, offspring, **kw)
    b.track()
    b.queue_targets_audio(tg)       # stored first, the objective after them
    b.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, FLOORS[1])
    got, stats = b.queue_run(0, 400, **rule)
    b.close()
    d = pkg.capi.SYNTH_DIMS[kind]
    es = pkg.HipES(parents, offspring, **kw)
    es.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, FLOORS[1])
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


# ---- 6. group -----------------------------------------------------------------------------------------------------------------
def test_group_sets_every_island(pkg, O):
    kw = dict(synth_kind=0, audio_log2=10, param_max=PMAX[0], seed=SEED, workgroup_size=32)
    g = pkg.HipGroup([0, 0], 4, 64, 192, migration_interval=1000, **kw)
    g.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, FLOORS[1])
    g.set_target_audio(target_audio(O, 0, 1024))
    g.init_population(0)
    g.execute_generations(1)
    g.synchronize()
    for i in range(2):
        isl = g.island(i)
        assert isl.objective == (pkg.capi.OBJECTIVE_LOG_MAGNITUDE, float(np.float32(FLOORS[1])))
        es = pkg.HipES(64, 192, gid_base=i * 256, **kw)
        es.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, FLOORS[1])
        es.set_target_audio(target_audio(O, 0, 1024))
        es.init_population(0)
        es.execute_generations(1)
        for name, x, y in zip(("values", "steps", "fitness"), isl.read_population(), es.read_population()):
            assert same_bits(x, y), (i, name)
        es.close()
    with pytest.raises(pkg.capi.SotsError) as err:
        g.set_objective(1, 0.0)
    assert "island 0" in str(err.value) and "outside 1e-30 .. 1" in str(err.value)
    g.close()


# ---- 8. elitist run -----------------------------------------------------------------------------------------------------------
def test_elitist_run_never_gets_worse(pkg, O):
    es = make(pkg, O, 0, 10, 1024, FLOORS[1])
    es.set_survivors(1)
    es.init_population(0)
    best = []
    for _ in range(200):
        es.execute_generations(1)
        best.append(float(es.read_fitness()[0]))
    es.close()
    print(f"row 0 under the log objective: generation 1 {best[0]:.6g}, generation 200 {best[-1]:.6g}")
    assert all(y <= x for x, y in zip(best, best[1:]))
    assert best[-1] < best[0]
