"""sots_render_continuous against its NumPy statement, tests/_render_continuous_model.py, BIT FOR BIT and
with no tolerance: the phases are sums of 32-bit integers, which are the same bits however they are tiled, and everything
in front of the sums is per-sample fp32 with one rounding per operation.

The device works in tiles of TILE = 4096 samples (kContTile, csrc/sots_render.h): a tile's increments are summed, the tile
totals are scanned by one workgroup, a lane per tile, and every tile is scanned again on top of its base."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_continuous_model as CM  # noqa: E402

pytestmark = pytest.mark.gpu

PMAX, DIMS, track_rows = CM.PMAX, CM.DIMS, CM.track_rows
SEED = 0x5EED0001
TILE = 4096
MAX_ROWS = 70


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def first_difference(got, want):
    if got.shape != want.shape:
        return "shapes %r and %r" % (got.shape, want.shape)
    d = np.flatnonzero(bits(got) != bits(want))
    return "equal" if d.size == 0 else "%d samples differ, first at %d: got %r want %r" % (d.size, d[0], got[d[0]], want[d[0]])


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


_ROWS = {}


def rows_of(kind):
    """the 70 rows of genes of a voice, made once (the corner rows of track_rows among them: negative increments and
    increments of 2^31 and more before the reduction, tests/test_render_continuous_cpu.py checks that on the model)"""
    if kind not in _ROWS:
        _ROWS[kind] = track_rows(kind, MAX_ROWS, 100 * kind + 8)
    return _ROWS[kind]


@pytest.fixture(scope="module")
def tab(O):
    return O.wavetable()


def context(pkg, kind, log2n, parents=32, offspring=32):
    return pkg.HipES(parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=32)


def model(kind, values, tab, n, hop, glide, **kw):
    return CM.render(kind, values, [0.0] * DIMS[kind], PMAX[kind], tab, n, hop, glide, **kw)


# ---- shapes: device == model --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 7, 70])
@pytest.mark.parametrize("log2n", [8, 10])
@pytest.mark.parametrize("kind", [0, 1, 3, 2])
def test_render_equals_the_model(pkg, tab, kind, log2n, rows):
    n = 1 << log2n
    values = rows_of(kind)[:rows]
    es = context(pkg, kind, log2n)
    for hop in (n, n // 4, 101, 1):
        for glide in (False, True):
            got = es.render_continuous(values, hop, glide=glide)
            want = model(kind, values, tab, n, hop, glide)
            assert got.shape == ((rows - 1) * hop + n,)
            assert same_bits(got, want), "hop %d glide %d: %s" % (hop, glide, first_difference(got, want))
    es.close()


# ---- the scan of the tile totals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,glide", [(1, False), (2, True)])
def test_scan_of_tile_totals_spans_more_than_a_wavefront(pkg, tab, kind, glide):
    """70 rows at N = 4096, hop = N: 286720 samples = 70 tiles of 4096, so the workgroup that scans the tile totals (a lane per
    tile) carries sums from its first wavefront (tiles 0..63) into its second"""
    n, rows = 4096, 70
    assert (rows * n) // TILE > 64
    values = rows_of(kind)
    es = context(pkg, kind, 12)
    got = es.render_continuous(values, n, glide=glide)
    want = model(kind, values, tab, n, n, glide)
    assert same_bits(got, want), first_difference(got, want)
    es.close()


# ---- passes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_result_does_not_depend_on_the_pass_size(pkg, tab, kind):
    n, rows = 1024, 70
    values = rows_of(kind)
    es = context(pkg, kind, 10)
    for hop, glide in ((256, False), (131, True)):
        want = model(kind, values, tab, n, hop, glide)
        assert len(want) > 2 * TILE  # several tiles and, below, several passes that end inside a tile
        for per_pass in (0, TILE - 1, TILE + 1):
            got = es.render_continuous(values, hop, glide=glide, samples_per_pass=per_pass)
            assert same_bits(got, want), "hop %d samples_per_pass %d: %s" % (hop, per_pass, first_difference(got, want))
    es.close()


# ---- output length -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1024, 256, 101])
def test_output_shorter_and_longer_than_the_rendering(pkg, tab, hop):
    kind, n, rows = 0, 1024, 7
    values = rows_of(kind)[:rows]
    covered = (rows - 1) * hop + n
    es = context(pkg, kind, 10)
    for per_pass in (0, 1000):
        for length in (covered - 5, covered + 5, 3, 0):
            got = es.render_continuous(values, hop, samples_per_pass=per_pass, out_samples=length)
            want = model(kind, values, tab, n, hop, False, out_samples=length)
            assert got.shape == (length,)
            assert same_bits(got, want), first_difference(got, want)
        got = es.render_continuous(values, hop, samples_per_pass=per_pass, out_samples=covered + 5)
        assert not bits(got[covered:]).any(), "the tail behind the rendering must be exactly +0"
    es.close()


# ---- context state ---------------------------------------------------------------------------------------------------------
def test_render_between_generations_leaves_the_run_alone(pkg, O):
    kind, log2n, n = 0, 10, 1024
    values = rows_of(kind)
    target = O.synth(0, [1450.0 / 3520.0, 3.0 / 8.0, 200.0 / 3520.0, 1.0], [0.0] * 4, PMAX[0], n)
    runs = []
    for render in (True, False):
        es = context(pkg, kind, log2n, 512, 1536)  # P = 2048: the selection with its lazy tail, splitters and lists
        es.track()
        es.set_target_audio(target)
        es.init_population(0)
        es.execute_generations(3)
        if render:
            es.render_continuous(values, n // 4, glide=True, samples_per_pass=5000)
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
def test_render_continuous_error_codes(pkg, hip):
    kind, n, rows = 1, 1024, 7
    v = np.ascontiguousarray(rows_of(kind)[:rows])
    es = context(pkg, kind, 10)
    L = hip.load()
    out = np.empty((rows - 1) * n + n, np.float32)

    def call(args, nbytes=v.nbytes, num_rows=rows, output=out):
        return L.sots_render_continuous(es._h, v.ctypes.data_as(C.c_void_p), nbytes, num_rows, args,
                                        output.ctypes.data_as(C.c_void_p) if output is not None else None, out.size)

    def args(hop=n, flags=0, per_pass=0, size=C.sizeof(hip.RenderContinuousArgs)):
        return C.byref(hip.RenderContinuousArgs(size, hop, flags, per_pass))

    INVALID, SIZE, STATE = -1, -4, -5
    assert call(args()) == 0
    assert call(args(flags=1)) == 0
    assert call(None) == INVALID                          # null args
    assert call(args(size=C.sizeof(hip.RenderContinuousArgs) - 4)) == INVALID
    assert call(args(size=C.sizeof(hip.RenderContinuousArgs) + 4)) == INVALID
    assert call(args(hop=0)) == INVALID                   # hop outside 1 .. N
    assert call(args(hop=n + 1)) == INVALID
    assert call(args(hop=1)) == 0
    assert call(args(flags=2)) == INVALID                 # unknown flag bits
    assert call(args(flags=3)) == INVALID
    assert call(args(), nbytes=0, num_rows=0) == INVALID  # no rows
    assert call(args(), nbytes=v.nbytes - 4) == SIZE
    assert call(args(), nbytes=v.nbytes + 24, num_rows=rows) == SIZE
    assert b"values" in L.sots_last_error(es._h)
    # S = (num_rows - 1) hop + N >= 2^31 is refused before the values are looked at
    assert call(args(hop=n), nbytes=(1 << 21) * 24, num_rows=1 << 21) == INVALID
    assert b"2^31" in L.sots_last_error(es._h)
    assert call(args(), output=None) == INVALID
    with pytest.raises(pkg.SotsError) as e:
        es.render_continuous(v, n + 1)
    assert e.value.code == INVALID
    es.set_synth_arithmetic(1)                            # the reference's device kernels' arithmetic: not this renderer's
    assert call(args()) == STATE
    assert b"SOTS_ARITH_DEVICE_KERNELS" in L.sots_last_error(es._h)
    es.set_synth_arithmetic(0)
    assert call(args()) == 0
    es.close()
