"""sots_render_overlap_add against its NumPy statement, tests/_render_model.py, BIT FOR BIT: the rows'
audio is the CPU oracle's, the sums are fp32 in ascending chunk order, the quotient is the correctly rounded one.  And
the hop forms of the batch's audio target setters against the spectra forms fed the explicit slices."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

PMAX = {0: [3520.0, 8.0, 3520.0, 1.0],
        1: [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0],
        3: [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0]}
DIMS = {0: 4, 1: 6, 3: 8}
SEED = 0x5EED0001
MAX_ROWS = 70


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def first_difference(got, want):
    d = np.flatnonzero(bits(got) != bits(want))
    return "equal" if d.size == 0 else "%d samples differ, first at %d: got %r want %r" % (d.size, d[0], got[d[0]], want[d[0]])


_ROWS = {}


def rows_of(O, kind, log2n, ocl=False):
    """the 70 rows of genes of a shape and their audio on the CPU oracle, made once"""
    key = (kind, log2n, ocl)
    if key not in _ROWS:
        values = M.unit_rows(MAX_ROWS, DIMS[kind], 100 * kind + log2n)
        _ROWS[key] = (values, M.oracle_rows(O, kind, values, [0.0] * DIMS[kind], PMAX[kind], 1 << log2n, ocl))
    return _ROWS[key]


def context(pkg, kind, log2n, parents=32, offspring=32):
    return pkg.HipES(parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=32)


def hops_of(n):
    return [n, n // 2, n // 4, 101, (n + 63) // 64]


# ---- shapes: device == model --------------------------------------------------------------------------------------------
SHAPES = [(0, 8), (0, 10), (1, 8), (1, 10)]


@pytest.mark.parametrize("rows", [1, 7, 70])
@pytest.mark.parametrize("kind,log2n", SHAPES)
def test_render_equals_the_model(pkg, O, kind, log2n, rows):
    n = 1 << log2n
    values, audio = rows_of(O, kind, log2n)
    w = M.window32(O, n)
    es = context(pkg, kind, log2n)
    for hop in hops_of(n):
        for windowed in (True, False):
            got = es.render_overlap_add(values[:rows], hop, windowed=windowed)
            want = M.overlap_add(audio[:rows], hop, w if windowed else None)
            assert got.shape == want.shape == ((rows - 1) * hop + n,)
            assert same_bits(got, want), "hop %d windowed %d: %s" % (hop, windowed, first_difference(got, want))
    es.close()


def test_render_four_operators_n2048(pkg, O):
    kind, log2n, n, rows = 3, 11, 2048, 70
    values, audio = rows_of(O, kind, log2n)
    w = M.window32(O, n)
    es = context(pkg, kind, log2n)
    for hop, windowed in ((n, False), (n // 4, True), (101, True), (32, True)):
        got = es.render_overlap_add(values[:rows], hop, windowed=windowed)
        want = M.overlap_add(audio[:rows], hop, w if windowed else None)
        assert same_bits(got, want), "hop %d windowed %d: %s" % (hop, windowed, first_difference(got, want))
    es.close()


# ---- passes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [7, 70])
def test_result_does_not_depend_on_the_pass_size(pkg, O, rows):
    kind, log2n, n = 0, 10, 1024
    values, audio = rows_of(O, kind, log2n)
    w = M.window32(O, n)
    es = context(pkg, kind, log2n)
    for hop in (n, n // 4, 101, 16):
        want = M.overlap_add(audio[:rows], hop, w)
        for per_pass in (0, 3, 1):
            got = es.render_overlap_add(values[:rows], hop, windowed=True, rows_per_pass=per_pass)
            assert same_bits(got, want), "hop %d rows_per_pass %d: %s" % (hop, per_pass, first_difference(got, want))
    es.close()


# ---- output length -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1024, 256, 101])
def test_output_shorter_and_longer_than_the_covered_range(pkg, O, hop):
    kind, log2n, n, rows = 0, 10, 1024, 7
    values, audio = rows_of(O, kind, log2n)
    w = M.window32(O, n)
    covered = (rows - 1) * hop + n
    es = context(pkg, kind, log2n)
    for per_pass in (0, 3):
        for length in (covered - 5, covered + 5):
            got = es.render_overlap_add(values[:rows], hop, windowed=True, rows_per_pass=per_pass, out_samples=length)
            want = M.overlap_add(audio[:rows], hop, w, out_samples=length)
            assert got.shape == (length,)
            assert same_bits(got, want), first_difference(got, want)
        assert not bits(got[covered:]).any(), "the tail behind the covered range must be exactly +0"
    es.close()


# ---- rectangular, hop = N: the rows end to end -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,log2n,arith", [(0, 10, 0), (1, 10, 0), (1, 10, 1)])
def test_rectangular_at_hop_n_is_the_rows_audio(pkg, O, kind, log2n, arith):
    n = 1 << log2n
    values, audio = rows_of(O, kind, log2n, ocl=bool(arith))
    values, audio = values[:64], audio[:64]
    es = context(pkg, kind, log2n)  # P = 64: the same rows the old way
    if arith:
        es.set_synth_arithmetic(arith)
    got = es.render_overlap_add(values, n, windowed=False)
    es.write_population(values=values)
    es.synthesise()
    old_way = es.read_audio()
    assert same_bits(got, old_way.reshape(-1)), first_difference(got, old_way.reshape(-1))
    assert same_bits(got, audio.reshape(-1)), first_difference(got, audio.reshape(-1))
    assert same_bits(got, M.overlap_add(audio, n))
    es.close()


# ---- context state ---------------------------------------------------------------------------------------------------------
def test_render_between_generations_leaves_the_run_alone(pkg, O):
    kind, log2n, n = 0, 10, 1024
    values, _ = rows_of(O, kind, log2n)
    target = O.synth(0, [1450.0 / 3520.0, 3.0 / 8.0, 200.0 / 3520.0, 1.0], [0.0] * 4, PMAX[0], n)
    runs = []
    for render in (True, False):
        es = context(pkg, kind, log2n, 512, 1536)  # P = 2048: the selection with its lazy tail, splitters and lists
        es.track()
        es.set_target_audio(target)
        es.init_population(0)
        es.execute_generations(3)
        if render:
            es.render_overlap_add(values, n // 4, windowed=True, rows_per_pass=16)
        assert es.generation == 3
        es.execute_generations(3)
        runs.append((es.read_population(), es.read_audio(), es.read_spectrum().view(np.float32), es.read_target(), es.best_ever(),
                     es.generation))
        es.close()
    (pa, aa, sa, ta, ba, ga), (pb, ab, sb, tb, bb, gb) = runs
    assert ga == gb == 6
    for name, x, y in zip(("values", "steps", "fitness"), pa, pb):
        assert same_bits(x, y), name
    assert same_bits(aa, ab) and same_bits(sa, sb) and same_bits(ta, tb)
    for x, y in zip(ba[:3], bb[:3]):
        assert same_bits(x, y)
    assert ba[3] == bb[3]


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_render_error_codes(pkg, O, hip):
    kind, log2n, n, rows = 0, 10, 1024, 7
    values, _ = rows_of(O, kind, log2n)
    v = np.ascontiguousarray(values[:rows])
    es = context(pkg, kind, log2n)
    L = hip.load()
    out = np.empty((rows - 1) * n + n, np.float32)

    def call(args, nbytes=v.nbytes, num_rows=rows):
        return L.sots_render_overlap_add(es._h, v.ctypes.data_as(C.c_void_p), nbytes, num_rows, args, out.ctypes.data_as(C.c_void_p), out.size)

    def args(hop=n, flags=1, per_pass=0, size=C.sizeof(hip.RenderArgs)):
        return C.byref(hip.RenderArgs(size, hop, flags, per_pass))

    INVALID, SIZE = -1, -4
    assert call(args()) == 0
    assert call(None) == INVALID                          # null args
    assert call(args(size=C.sizeof(hip.RenderArgs) - 4)) == INVALID
    assert call(args(size=C.sizeof(hip.RenderArgs) + 4)) == INVALID
    assert call(args(hop=(n + 63) // 64 - 1)) == INVALID  # hop outside ceil(N/64) .. N
    assert call(args(hop=0)) == INVALID
    assert call(args(hop=n + 1)) == INVALID
    assert call(args(hop=(n + 63) // 64)) == 0
    assert call(args(flags=2)) == INVALID                 # unknown flag bits
    assert call(args(flags=3)) == INVALID
    assert call(args(), nbytes=0, num_rows=0) == INVALID  # no rows
    assert call(args(), nbytes=v.nbytes - 4) == SIZE
    assert call(args(), nbytes=v.nbytes + 16, num_rows=rows) == SIZE
    assert b"values" in L.sots_last_error(es._h)
    with pytest.raises(pkg.SotsError) as e:
        es.render_overlap_add(values[:rows], n + 1)
    assert e.value.code == INVALID
    es.close()


# ---- hop on the batch's audio target setters ---------------------------------------------------------------------------------
def hop_signal(samples):
    t = np.arange(samples) / 44100.0
    rng = np.random.default_rng(77)
    f = 180.0 + 400.0 * t / t[-1]  # a glide: every slice has a spectrum of its own
    return (0.6 * np.sin(2 * np.pi * f * t) + 0.3 * np.sin(2 * np.pi * 2.7 * f * t) + 0.05 * rng.standard_normal(samples)).astype(np.float32)


def hop_batch(pkg, chunks):
    b = pkg.HipBatch(chunks, 16, 16, synth_kind=0, audio_log2=10, param_max=PMAX[0], seed=SEED, workgroup_size=16)
    b.track()
    return b


def batch_run(b, chunks, gens=20):
    b.init_population(0)
    b.execute_generations(gens)
    return [b.read_population(c) for c in range(chunks)]


def assert_same_populations(x, y):
    assert len(x) == len(y)
    for c, (p, q) in enumerate(zip(x, y)):
        for name, u, v in zip(("values", "steps", "fitness"), p, q):
            assert same_bits(u, v), "chunk %d: %s differ" % (c, name)


def assert_same_results(x, y):
    assert len(x) == len(y)
    for name in x.dtype.names:
        assert np.array_equal(np.ascontiguousarray(x[name]).view(np.uint32), np.ascontiguousarray(y[name]).view(np.uint32)), name


@pytest.mark.parametrize("hop", [512, 1024])
def test_hop_setters_equal_the_spectra_of_the_slices(pkg, O, hop):
    n, chunks, gens = 1024, 8, 20
    audio = hop_signal((chunks - 1) * hop + n + 37)  # (samples behind the last chunk are not a chunk)
    mags = np.stack([O.spectrum(audio[k * hop:k * hop + n]) for k in range(chunks)])
    b = hop_batch(pkg, chunks)
    b.set_target_spectra(mags)
    want = batch_run(b, chunks, gens)
    b.set_target_audio(audio, hop=hop)
    assert b.active == chunks
    assert_same_populations(batch_run(b, chunks, gens), want)
    b.queue_targets_spectra(mags)
    want_q, _ = b.queue_run(0, gens)
    b.queue_targets_audio(audio, hop=hop)
    assert b.queued == chunks
    got_q, _ = b.queue_run(0, gens)
    assert_same_results(got_q, want_q)
    if hop == n:  # the existing entry points are the hop = N case
        b.set_target_audio(audio[:chunks * n])
        assert_same_populations(batch_run(b, chunks, gens), want)
        b.queue_targets_audio(audio[:chunks * n])
        got_q, _ = b.queue_run(0, gens)
        assert_same_results(got_q, want_q)
    b.close()


def test_hop_setters_refuse(pkg):
    n, chunks = 1024, 4
    b = hop_batch(pkg, chunks)
    audio = hop_signal(3 * 512 + n)
    L = b.L
    p = audio.ctypes.data_as(C.c_void_p)
    INVALID, SIZE = -1, -4
    assert L.sots_batch_set_target_audio_hop(b._h, p, audio.size, 512, chunks) == 0
    assert L.sots_batch_set_target_audio_hop(b._h, p, audio.size - 1, 512, chunks) == SIZE
    assert L.sots_batch_set_target_audio_hop(b._h, p, audio.size, 0, chunks) == INVALID
    assert L.sots_batch_set_target_audio_hop(b._h, p, audio.size, n + 1, chunks) == INVALID
    assert L.sots_batch_queue_targets_audio_hop(b._h, p, audio.size, 512, chunks) == 0
    assert L.sots_batch_queue_targets_audio_hop(b._h, p, audio.size - 1, 512, chunks) == SIZE
    assert L.sots_batch_queue_targets_audio_hop(b._h, p, audio.size, 0, chunks) == INVALID
    assert L.sots_batch_queue_targets_audio_hop(b._h, p, audio.size, n + 1, chunks) == INVALID
    b.close()
