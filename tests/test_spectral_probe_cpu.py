"""The probes of tests/_spectral_probe.py have power: on the fp64 model, every single fault of every class moves some probe
row by at least 4 x that row's bound under one of the sparse targets - for every (N, objective, weights) combination
that tests/test_gpu_spectral_probe.py runs.  No GPU: the device tests hold the kernels inside 1 x the bound, this one
shows that no pairing mistake fits inside 4 x."""
import numpy as np
import pytest

import _spectral_probe as sp

LOG2NS = (8, 9, 10, 11, 12, 13, 14, 15)
# the segmented shapes of the GPU tests: (log2 N, chunks, rows per chunk)
BATCHES = [(9, 3, 64), (10, 3, 64), (10, 3, 1024), (8, 4, 16), (11, 4, 16), (12, 4, 16), (13, 4, 16), (11, 4, 1024), (12, 4, 1024),
           (14, 4, 16)]
SEED = 0x5EED0001
_M = {}


def tone_magnitudes(O, log2n):
    if log2n not in _M:
        _M.clear()                                            # (one N at a time: 2048 x 4097 doubles at N = 8192)
        _M[log2n] = sp.tone_magnitudes(O, 1 << log2n)
    return _M[log2n]


def case(O, log2n, eps, weighted, targets=3):
    n = 1 << log2n
    w = sp.probe_weights(n) if weighted else None
    return sp.Power(n, tone_magnitudes(O, log2n), sp.sparse_targets(n, targets), w, eps, sp.relative_term(log2n, weighted)), w


def test_the_relative_term_is_below_the_design_figure():
    for log2n in LOG2NS:
        assert 5e-7 < sp.relative_term(log2n, False) < sp.relative_term(log2n, True) < 2e-5
    assert sp.sum_depth(9) == 10 and sp.sum_depth(10) == 12 and sp.sum_depth(8) == 9 and sp.sum_depth(13) == 71 and sp.sum_depth(15) == 47


def test_probe_inputs_are_what_the_design_says():
    for log2n in LOG2NS:
        n = 1 << log2n
        t, w = sp.sparse_targets(n, 4), sp.probe_weights(n)
        bins = sp.probed_bins(n)
        for j in range(4):
            nz = np.flatnonzero(t[j])
            assert np.array_equal(nz, bins[bins % 3 == j % 3]) and t[j][nz].min() >= 0.05 and t[j][nz].max() <= 0.25
        assert t[0][0] >= 0.05 and np.all(t[0][t[0] != 0] != t[3][t[0] != 0])        # a loud DC bin; a fourth table differs wherever it is loud
        assert w.min() >= 0.25 and w.max() <= 1.75
        pr = sp.pairs(n)
        assert np.abs(w[pr[:, 0]] - w[pr[:, 1]]).min() >= 0.29
        # k and k + 2^s are loud in different targets (outside the bands of the large sizes: in none)
        one_sided = np.sum((t[:3][:, pr[:, 0]] != 0) != (t[:3][:, pr[:, 1]] != 0), axis=0)
        assert np.all(one_sided == 2) if log2n < sp.BAND_FROM else np.all(one_sided >= 1)
        v, s = sp.probe_rows(n, 2 * sp.tone_bins(n).size + 5)
        assert v.dtype == np.float32 and np.all(v[:, 1] == 0) and np.all((v[:, 3] >= 0.5) & (v[:, 3] <= 1.0)) and np.all(v[:, 2] < 1.0)
        assert np.unique(v, axis=0).shape[0] == v.shape[0] and np.all(s == np.float32(sp.STEP))
        assert sp.tone_bins(n).size == (n // 4 if log2n < 14 else 384)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights"])
@pytest.mark.parametrize("eps", sp.OBJECTIVES, ids=["magnitude", "log"])
@pytest.mark.parametrize("log2n", LOG2NS)
def test_every_single_fault_moves_a_probe_row_by_four_bounds(O, log2n, eps, weighted):
    n = 1 << log2n
    power, _ = case(O, log2n, eps, weighted)
    bins, pr = sp.probed_bins(n), sp.pairs(n)
    shown = {"(a) bin left out": power.left_out(bins), "(b) bin counted twice": power.counted_twice(bins),
             "(c) target entries exchanged": power.exchanged(pr, "targets"), "(e) Nyquist bin added / for bin 0 / for bin N/4": power.nyquist()}
    if weighted:
        shown["(d) weight entries exchanged"] = power.exchanged(pr, "weights")
    print(f"N {n} {'magnitude' if eps is None else 'log, floor %g' % eps}{', weights' if weighted else ''}: r {sp.relative_term(log2n, weighted):.3g}; "
          + "; ".join(f"{k}: {int(v.sum())} of {v.size}" for k, v in shown.items()))
    assert shown["(c) target entries exchanged"].size == sum(np.count_nonzero(np.isin(np.arange(n // 2 - d), bins) | np.isin(np.arange(d, n // 2), bins))
                                                             for d in sp.strides(n // 2))
    for name, v in shown.items():
        assert v.all(), (name, int((~v).sum()), np.flatnonzero(~v)[:8])


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights"])
@pytest.mark.parametrize("eps", sp.OBJECTIVES, ids=["magnitude", "log"])
@pytest.mark.parametrize("log2n", [8, 10])
def test_the_closed_forms_are_the_faults_applied_to_the_model(O, log2n, eps, weighted):
    """a seeded sample of every class: the model with the fault applied (faulty_fitness) moves the rows by what Power works
    out slot by slot, and under MAGNITUDE without weights an exchange of targets k, k' changes F by 2 (m_k - m_k') (t_k - t_k')"""
    n, half = 1 << log2n, (1 << log2n) // 2
    power, w = case(O, log2n, eps, weighted)
    m, t = power.m, sp.sparse_targets(n)
    rng = np.random.default_rng(log2n)
    pr = sp.pairs(n)
    sample = pr[rng.choice(pr.shape[0], 12, replace=False)]
    for j in range(3):
        f0 = sp.faulty_fitness(None, m, t[j], w, eps)
        np.testing.assert_allclose(f0, sp.fitness(m[:, :-1], t[j], w, eps), rtol=1e-13)
        need = sp.POWER * sp.bound(m[:, :-1], t[j], w, eps, sp.relative_term(log2n, weighted))
        np.testing.assert_allclose(need, power.need[j], rtol=1e-13)
        for k, k2 in sample:
            k, k2 = int(k), int(k2)
            rows = np.concatenate([power.rows_near([k]), power.rows_near([k2])], axis=1)
            df = sp.faulty_fitness(sp.targets_exchanged(k, k2), m, t[j], w, eps) - f0
            if eps is None and not weighted:
                np.testing.assert_allclose(df, 2 * (m[:, k] - m[:, k2]) * (np.float64(t[j][k]) - np.float64(t[j][k2])), rtol=1e-9, atol=1e-11)
            one = np.array([[k, k2]])
            got = {"targets": df, "weights": sp.faulty_fitness(sp.weights_exchanged(k, k2), m, t[j], w, eps) - f0}
            for which, want in got.items():
                only_j = sp.Power(n, m, t[j:j + 1], w, eps, sp.relative_term(log2n, weighted))
                assert only_j.exchanged(one, which)[0] == bool(np.any(np.abs(want[rows]) >= need[rows])), (which, k, k2)
            only_j = sp.Power(n, m, t[j:j + 1], w, eps, sp.relative_term(log2n, weighted))
            d_out = sp.faulty_fitness(sp.left_out(k), m, t[j], w, eps) - f0
            d_twice = sp.faulty_fitness(sp.counted_twice(k), m, t[j], w, eps) - f0
            np.testing.assert_allclose(d_out, -d_twice, rtol=1e-9, atol=1e-11)
            near = power.rows_near([k])
            assert only_j.left_out(np.array([k]))[0] == bool(np.any(np.abs(d_out[near]) >= need[near]))
        nyq = [sp.faulty_fitness(f, m, t[j], w, eps) - f0 for f in (sp.nyquist_added(half), sp.nyquist_in_place_of(0, half), sp.nyquist_in_place_of(half // 2, half))]
        only_j = sp.Power(n, m, t[j:j + 1], w, eps, sp.relative_term(log2n, weighted))
        assert only_j.nyquist().tolist() == [bool(np.any(np.abs(d) >= need)) for d in nyq]


def test_the_image_of_the_long_row_kernel_holds_every_bin_once():
    for log2n in (8, 11, 12, 13):
        n = 1 << log2n
        bins = sp.x_image_bins(n)
        assert bins.shape == (64, n // 128) and np.array_equal(np.sort(bins.reshape(-1)), np.arange(n // 2))
        assert np.array_equal(bins[:, 0], (n // 128) * np.array([int(f"{l:06b}"[::-1], 2) for l in range(64)]))   # register 0: the lane's first bin
        t = sp.sparse_targets(n, 4)
        assert np.array_equal(sp.x_table_read_late(t, 0), t[0])                                               # chunk 0 reads its own table
        assert not np.array_equal(sp.x_table_read_late(t, 1), t[1])


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weights"])
@pytest.mark.parametrize("eps", sp.OBJECTIVES, ids=["magnitude", "log"])
@pytest.mark.parametrize("log2n,chunks,rows", BATCHES)
def test_a_segmented_launch_that_takes_the_wrong_table_shows(O, log2n, chunks, rows, eps, weighted):
    """(f) chunk c judged against chunk c' != c's table, (g) chunk c >= 1's table read c entries late: each moves one of
    the chunk's own first rows - the tones a batch draws in the box TONE_PMAX, at most 32 of them - by 4 bounds"""
    n = 1 << log2n
    w = sp.probe_weights(n) if weighted else None
    r = sp.relative_term(log2n, weighted)
    tables = sp.sparse_targets(n, chunks)
    worst = np.inf
    for c in range(chunks):
        v, _ = O.init_population(rows, 4, SEED, 0, c)
        m = sp.magnitudes_ext(O, sp.synthesise(O, v[:32], n, sp.TONE_PMAX))[:, :-1]
        f0 = sp.fitness(m, tables[c], w, eps)
        need = sp.POWER * sp.bound(m, tables[c], w, eps, r)
        wrong = [(f"(f) {c} <- {c2}", sp.other_chunks_table(tables, c2)) for c2 in range(chunks) if c2 != c]
        if c:
            wrong.append((f"(g) {c}", sp.table_read_late(tables, c)))
            if log2n in (8, 11, 12, 13):                      # k_fft_x reads its chunk's table from the permuted image
                wrong.append((f"(g) {c}, image", sp.x_table_read_late(tables, c)))
        for name, t in wrong:
            moved = np.max(np.abs(sp.fitness(m, t, w, eps) - f0) / need)
            worst = min(worst, moved)
            assert moved >= 1.0, (name, moved)
    print(f"N {n}, {chunks} x {rows}: the least visible wrong table moves a row by {sp.POWER * worst:.3g} bounds")
