"""Every bin of the spectral fitness kernels against fp64 (tests/_spectral_probe.py): tone rows, sparse targets and
weights under which a bin left out, a bin counted twice, two exchanged entries of the target or weight table, the Nyquist
bin in the sum or a chunk judged against another chunk's table moves some row by more than 4 x its bound
(tests/test_spectral_probe_cpu.py shows that on the model, for every case below).  Here every row must be within 1 x
the bound: sum_k w_k (2 |e_k| d_k + d_k^2) + r F with r from the kernel's own summation order, not the project's 1e-4.

Each case prints a line `PROBE {...}` with its worst |dF| / bound; profiles/r17_spectral_probe.json collects them.

The shapes are the smallest that reach each kernel form on 256 CUs (spectral_choice, csrc/sots_kernels.hip): one wavefront
per row (N = 512, 1024), the wide form (N = 1024 from 3072 rows), k_fft_x with four wavefronts (fewer than 4081 rows) and
with sixteen or eight, a workgroup per row (N = 16 384, 32 768: the banded tone set)."""
import json

import numpy as np
import pytest

import _spectral_probe as sp

pytestmark = pytest.mark.gpu

SEED = 0x5EED0001
OFFSPRING = 32            # the fused cases: the probe rows are the parents, all of them survivors
JUDGE_ALL = 1 << 23       # rows x bins up to which the model judges every row; beyond, the tone set once and SAMPLE repeats
SAMPLE = 256
BATCH_ROWS = 512          # rows of a batch the model judges, over its chunks

# (form, log2 N, rows)
FORMS = [("wave", 9, 128), ("wave", 10, 256), ("wide", 10, 3072), ("x_small", 8, 64), ("x_small", 11, 512), ("x_small", 12, 1024),
         ("x_small", 13, 2048), ("x", 8, 4096), ("x", 11, 4096), ("x", 12, 4096), ("x", 13, 4096), ("big", 14, 384), ("big", 15, 384)]
# (form of the batch's launch, log2 N, chunks, parents, offspring)
BATCHES = [("wave", 9, 3, 16, 48), ("wave", 10, 3, 16, 48), ("wide", 10, 3, 256, 768), ("x_small", 8, 4, 4, 12), ("x_small", 11, 4, 4, 12),
           ("x_small", 12, 4, 4, 12), ("x_small", 13, 4, 4, 12), ("x", 11, 4, 256, 768), ("x", 12, 4, 256, 768), ("big", 14, 4, 4, 12)]
CASES = [(eps, weighted) for eps in sp.OBJECTIVES for weighted in (False, True)]
CASE_IDS = [f"{'magnitude' if eps is None else 'log'}-{'weights' if weighted else 'plain'}" for eps, weighted in CASES]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def set_objective(pkg, es, eps, weights):
    if eps is None:
        es.set_objective(pkg.capi.OBJECTIVE_MAGNITUDE)
    else:
        es.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, eps)
    es.set_objective_weights(weights)


def judged_rows(n, rows):
    """every row, or (rows x bins beyond JUDGE_ALL - the sixteen-wavefront form at N = 8192) the tone set once and a seeded
    sample of its repeats: the fp64 model of 4096 rows of 8192 samples under twelve settings takes too long for a test"""
    tones = sp.tone_bins(n).size
    if rows * (n // 2) <= JUDGE_ALL or rows <= tones + SAMPLE:
        return np.arange(rows)
    return np.concatenate([np.arange(tones), tones + np.sort(np.random.default_rng(n).choice(rows - tones, SAMPLE, replace=False))])


class RowModel:
    """fp64 magnitudes [N/2 + 1] (the Nyquist bin last) of rows by their genes, through the oracle's synthesis - bit-exact
    with the device's, which test_staged_fitness_of_the_probe_rows checks - and its fp64 transform; every row once per N and box"""
    held = {}

    @classmethod
    def of(cls, O, n, pmax):
        key = (n, tuple(pmax))
        if key not in cls.held:
            cls.held.clear()                                   # (one N at a time)
            cls.held[key] = cls(O, n, pmax)
        return cls.held[key]

    def __init__(self, O, n, pmax):
        self.O, self.n, self.pmax, self.rows = O, n, pmax, {}

    def magnitudes(self, values):
        values = np.ascontiguousarray(values, np.float32)
        keys = [v.tobytes() for v in values]
        new = {k: i for i, k in enumerate(keys) if k not in self.rows}
        if new:
            idx = np.fromiter(new.values(), int)
            for k, m in zip(new, sp.magnitudes_ext(self.O, sp.synthesise(self.O, values[idx], self.n, self.pmax))):
                self.rows[k] = m
        return np.stack([self.rows[k] for k in keys])


def check(f, m, t, w, eps, r, **case):
    """every row of f within its bound of the model; prints the worst |dF| / bound"""
    ratio, want = sp.judge(f, m, t, w, eps, r)
    worst = int(np.argmax(ratio))
    print("PROBE " + json.dumps({**case, "worst_dF_over_bound": float(f"{ratio[worst]:.4g}")}))
    assert np.all(np.isfinite(f)), case
    assert np.all(ratio <= 1.0), (case, worst, float(f[worst]), float(want[worst]), float(ratio[worst]), int(np.count_nonzero(ratio > 1.0)))


# ---- 1. the staged kernels: k_fft / k_fft_x / k_fft_big as spectrum writers, k_fitness / k_fitness_x / k_fitness_big ----------------
@pytest.mark.parametrize("form,log2n,rows", FORMS)
def test_staged_fitness_of_the_probe_rows(pkg, O, form, log2n, rows):
    """one synthesis and one transform of the probe rows, then fitness() under both objectives, with and without weights,
    against each of the three targets; the model's magnitudes come from the device's own audio"""
    n = 1 << log2n
    v, s = sp.probe_rows(n, rows)
    targets = sp.sparse_targets(n)
    es = pkg.HipES(rows // 2, rows - rows // 2, synth_kind=0, audio_log2=log2n, param_max=sp.PMAX, seed=SEED, workgroup_size=32)
    es.set_target_spectrum(targets[0])
    es.write_population(v, s)
    es.synthesise()
    pick = judged_rows(n, rows)
    audio = es.read_audio()[pick]
    # what lets the fused cases below judge a row by its genes: tones up to 22 050 Hz are the oracle's, bit for bit
    some = np.unique(np.concatenate([[0, pick.size - 1], np.random.default_rng(log2n).choice(pick.size, 14)]))
    assert same_bits(audio[some], sp.synthesise(O, v[pick][some], n))
    m = sp.magnitudes_ext(O, audio)[:, :-1]
    es.window(); es.fft()
    for eps, weighted in CASES:
        w = sp.probe_weights(n) if weighted else None
        set_objective(pkg, es, eps, w)
        for j, t in enumerate(targets):
            es.set_target_spectrum(t)
            es.fitness()
            check(es.read_fitness()[pick], m, t, w, eps, sp.relative_term(log2n, weighted),
                  path="staged", form=form, N=n, rows=rows, objective="magnitude" if eps is None else "log", weights=weighted, target=j)
    es.close()


# ---- 2. the fused kernels: no spectrum in memory, k_fft_x from the permuted table image -------------------------------------------
@pytest.mark.parametrize("eps,weighted", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("form,log2n,rows", FORMS)
def test_fused_generation_judges_the_probe_rows(pkg, O, form, log2n, rows, eps, weighted):
    """the probe rows as parents that all survive (bit copies through variation) beside 32 offspring of theirs, one fused
    generation per target: every returned row against the model of its own genes, and every probe row among them"""
    n = 1 << log2n
    v, s = sp.probe_rows(n, rows + OFFSPRING)
    w = sp.probe_weights(n) if weighted else None
    r = sp.relative_term(log2n, weighted)
    model = RowModel.of(O, n, sp.PMAX)
    probe = {row.tobytes(): i for i, row in enumerate(v[:rows])}
    pick = set(judged_rows(n, rows).tolist())
    es = pkg.HipES(rows, OFFSPRING, synth_kind=0, audio_log2=log2n, param_max=sp.PMAX, seed=SEED, workgroup_size=32)
    set_objective(pkg, es, eps, w)
    es.set_survivors(rows)
    for j, t in enumerate(sp.sparse_targets(n)):
        es.set_target_spectrum(t)
        es.write_population(v, s)
        es.generation = 0                                       # the same offspring under every target and setting
        es.execute_generations(1)
        gv, _, gf = es.read_population()
        keys = [row.tobytes() for row in gv]
        assert set(probe) <= set(keys), "a survivor is missing from the new population"
        judged = np.array([i for i, k in enumerate(keys) if k not in probe or probe[k] in pick])
        check(gf[judged], model.magnitudes(gv[judged])[:, :-1], t, w, eps, r,
              path="fused", form=form, N=n, rows=rows + OFFSPRING, objective="magnitude" if eps is None else "log", weights=weighted, target=j)
    es.close()


# ---- 3. list mode: the bucketing instantiation of the wide kernel -----------------------------------------------------------------
@pytest.mark.parametrize("eps,weighted", CASES, ids=CASE_IDS)
def test_list_mode_judges_an_evolving_probe_population(pkg, O, eps, weighted):
    """N = 1024, 4096 + 12288: from generation 2 AUTO files the keys in the spectral kernel.  Three generations from the
    probe population under AUTO and under TILES: the same bits, and every row of the final population within the bound of
    the model of its genes.  The rows evolve, so their power is printed, not asserted."""
    n, parents, offspring = 1024, 4096, 12288
    v, s = sp.probe_rows(n, parents + offspring)
    w = sp.probe_weights(n) if weighted else None
    r = sp.relative_term(10, weighted)
    t = sp.sparse_targets(n)[0]
    pops = []
    for plan in (pkg.capi.SELECT_AUTO, pkg.capi.SELECT_TILES):
        es = pkg.HipES(parents, offspring, synth_kind=0, audio_log2=10, param_max=sp.PMAX, seed=SEED, workgroup_size=32)
        set_objective(pkg, es, eps, w)
        es.set_target_spectrum(t)
        es.set_select_plan(plan)
        es.write_population(v, s)
        es.execute_generations(3)
        pops.append(es.read_population())
        es.close()
    for name, x, y in zip(("values", "steps", "fitness"), *pops):
        assert same_bits(x, y), name
    gv, _, gf = pops[0]
    m = RowModel(O, n, sp.PMAX).magnitudes(gv)                  # (not held: every case ends with other rows)
    check(gf, m[:, :-1], t, w, eps, r, path="list", form="wide+lists", N=n, rows=parents + offspring,
          objective="magnitude" if eps is None else "log", weights=weighted, target=0)
    power = sp.Power(n, m, t[None, :], w, eps, r)
    bins, pr = sp.probed_bins(n), sp.pairs(n)
    share = {"left out": power.left_out(bins).mean(), "targets exchanged": power.exchanged(pr, "targets").mean(), "nyquist": power.nyquist().mean()}
    if weighted:
        share["weights exchanged"] = power.exchanged(pr, "weights").mean()
    print("share of single faults the final population would show under this one target: " + ", ".join(f"{k} {100 * x:.1f} %" for k, x in share.items()))


# ---- 4. segmented launches: every row against its chunk's table -------------------------------------------------------------------
@pytest.mark.parametrize("eps,weighted", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("form,log2n,chunks,parents,offspring", BATCHES)
def test_batch_judges_every_chunk_against_its_own_table(pkg, O, form, log2n, chunks, parents, offspring, eps, weighted):
    """a batch draws its own rows, so the box makes every individual a tone (index 0 .. 0, carrier 0 .. 22 050 Hz); chunk c
    against the sparse target c.  After one generation each chunk is, bit for bit, a sequential context of the same box,
    target and init_population(c), and up to 512 seeded rows are within the bound of the model of their genes"""
    n, p = 1 << log2n, parents + offspring
    kw = dict(synth_kind=0, audio_log2=log2n, param_min=[0.0] * 4, param_max=sp.TONE_PMAX, seed=SEED, workgroup_size=16)
    w = sp.probe_weights(n) if weighted else None
    r = sp.relative_term(log2n, weighted)
    tables = sp.sparse_targets(n, chunks)
    b = pkg.HipBatch(chunks, parents, offspring, **kw)
    set_objective(pkg, b, eps, w)
    b.set_target_spectra(tables)
    b.init_population(0)
    b.execute_generations(1)
    b.synchronize()
    es = pkg.HipES(parents, offspring, **kw)
    set_objective(pkg, es, eps, w)
    model = RowModel.of(O, n, sp.TONE_PMAX)
    rng = np.random.default_rng(SEED + log2n)
    for c in range(chunks):
        es.set_target_spectrum(tables[c])
        es.init_population(c)
        es.execute_generations(1)
        got = b.read_population(c)
        for name, x, y in zip(("values", "steps", "fitness"), got, es.read_population()):
            assert same_bits(x, y), (c, name)
        pick = np.sort(rng.choice(p, min(p, BATCH_ROWS // chunks), replace=False))
        check(got[2][pick], model.magnitudes(got[0][pick])[:, :-1], tables[c], w, eps, r,
              path="batch", form=form, N=n, rows=chunks * p, objective="magnitude" if eps is None else "log", weights=weighted, target=c)
    es.close(); b.close()
