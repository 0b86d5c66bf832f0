"""sots_render_graph_continuous against its NumPy statement, tests/_render_graph_continuous_model.py, BIT FOR
BIT and with no tolerance: the phases are sums of 32-bit integers, which are the same bits however they are tiled, and
everything in front of the sums is per-sample fp32 with one rounding per operation.

The device works in tiles of TILE = 4096 samples, level by level of the graph: a tile's increments are summed, the tile totals
are scanned by one workgroup per operator, a lane per tile, and every tile is scanned again on top of its base; a last launch
mixes the carriers.  tests/test_render_graph_continuous_cpu.py asserts on the model what the rows used here cover."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _graph_waveforms_model as WM  # noqa: E402
import _render_continuous_model as CM  # noqa: E402
import _render_graph_continuous_model as GM  # noqa: E402

pytestmark = pytest.mark.gpu

GRAPHS = GM.GRAPHS
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


def rows_of(ops):
    """the 70 rows of genes for a graph of `ops` operators, made once; the first 7 are the rows whose coverage the CPU tests assert"""
    if ops not in _ROWS:
        _ROWS[ops] = GM.graph_rows(ops, MAX_ROWS, 100 + ops)
        assert np.array_equal(_ROWS[ops][:7], GM.graph_rows(ops, 7, 100 + ops))
    return _ROWS[ops]


@pytest.fixture(scope="module")
def tab(O):
    return O.wavetable()


def context(pkg, name, log2n, ranges=None, waves=None, parents=32, offspring=32):
    pmin, pmax = ranges or WM.ranges(GRAPHS[name][0])
    return pkg.HipES(parents, offspring, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=log2n, param_min=pmin, param_max=pmax, seed=SEED,
                     workgroup_size=32, graph=pkg.capi.make_voice_graph(*GRAPHS[name]), waveforms=waves)


def model(name, values, tab, n, hop, glide, ranges=None, waves=None, **kw):
    pmin, pmax = ranges or WM.ranges(GRAPHS[name][0])
    return GM.render(GRAPHS[name], waves, values, pmin, pmax, tab, n, hop, glide, **kw)


# ---- every graph: device == model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_every_graph_equals_the_model(pkg, tab, name):
    """N = 256, 7 rows, hop 101: S = 862 samples, no multiple of 4, so the quad that the pass's end cuts is exercised"""
    n, rows, hop = 256, 7, 101
    values = rows_of(GRAPHS[name][0])[:rows]
    es = context(pkg, name, 8)
    for glide in (False, True):
        got = es.render_graph_continuous(values, hop, glide=glide)
        want = model(name, values, tab, n, hop, glide)
        assert got.shape == (862,)
        assert same_bits(got, want), "glide %d: %s" % (glide, first_difference(got, want))
        assert np.abs(want).max() > 0.01
    es.close()


# ---- shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 7, 70])
@pytest.mark.parametrize("log2n", [8, 10])
@pytest.mark.parametrize("name", ["dense8", "stacks5", "one_mod_two_carriers"])
def test_render_equals_the_model(pkg, tab, name, log2n, rows):
    n = 1 << log2n
    values = rows_of(GRAPHS[name][0])[:rows]
    es = context(pkg, name, log2n)
    for hop in (n, n // 4, 101, 1):
        for glide in (False, True):
            got = es.render_graph_continuous(values, hop, glide=glide)
            want = model(name, values, tab, n, hop, glide)
            assert got.shape == ((rows - 1) * hop + n,)
            assert same_bits(got, want), "hop %d glide %d: %s" % (hop, glide, first_difference(got, want))
    es.close()


# ---- non-finite modulator outputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_mods", "chain8"])
def test_non_finite_modulator_outputs(pkg, tab, name):
    ops = GRAPHS[name][0]
    ranges = WM.overflow_ranges(ops)
    values = rows_of(ops)[:7]
    es = context(pkg, name, 8, ranges=ranges)
    for glide in (False, True):
        got = es.render_graph_continuous(values, 101, glide=glide)
        want = model(name, values, tab, 256, 101, glide, ranges=ranges)
        assert same_bits(got, want), "glide %d: %s" % (glide, first_difference(got, want))
        assert np.isfinite(got).all()
    es.close()


# ---- waveforms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", list(WM.WAVES))
def test_every_waveform_as_modulator_and_as_carrier(pkg, tab, w):
    waves = GM.chain3_waves(w)
    values = rows_of(3)[:7]
    es = context(pkg, "chain3", 8, waves=waves)
    for glide in (False, True):
        got = es.render_graph_continuous(values, 101, glide=glide)
        want = model("chain3", values, tab, 256, 101, glide, waves=waves)
        assert same_bits(got, want), "glide %d: %s" % (glide, first_difference(got, want))
    es.close()


def test_mixed_waveforms_on_dense8(pkg, tab):
    values = rows_of(8)[:7]
    es = context(pkg, "dense8", 8, waves=GM.MIXED8)
    for hop, glide in ((101, False), (64, True)):
        got = es.render_graph_continuous(values, hop, glide=glide)
        want = model("dense8", values, tab, 256, hop, glide, waves=GM.MIXED8)
        assert same_bits(got, want), "hop %d: %s" % (hop, first_difference(got, want))
    # the setting is read at the call: back to all sine
    es.set_voice_waveforms(None)
    assert same_bits(es.render_graph_continuous(values, 101), model("dense8", values, tab, 256, 101, False))
    es.close()


def test_levels_without_a_table_read(pkg, tab):
    """SQUARE and SAW modulators: the levels above 0 run without the table in LDS; the sine carriers' mix reads it"""
    waves = [6, 7, 0, 7, 0]
    values = rows_of(5)[:7]
    es = context(pkg, "stacks5", 8, waves=waves)
    got = es.render_graph_continuous(values, 101, glide=True)
    want = model("stacks5", values, tab, 256, 101, True, waves=waves)
    assert same_bits(got, want), first_difference(got, want)
    es.set_voice_waveforms([6, 7, 6, 7, 7])  # ... and a mix without it
    got = es.render_graph_continuous(values, 101)
    want = model("stacks5", values, tab, 256, 101, False, waves=[6, 7, 6, 7, 7])
    assert same_bits(got, want), first_difference(got, want)
    es.close()


# ---- the scan of the tile totals ---------------------------------------------------------------------------------------------
def test_scan_of_tile_totals_spans_more_than_a_wavefront(pkg, tab):
    """70 rows at N = 4096, hop = N: 286720 samples = 70 tiles of 4096, so the workgroup that scans an operator's tile totals (a
    lane per tile) carries sums from its first wavefront (tiles 0..63) into its second"""
    n, rows = 4096, 70
    assert (rows * n) // TILE > 64
    values = rows_of(5)
    es = context(pkg, "stacks5", 12)
    got = es.render_graph_continuous(values, n, glide=True)
    want = model("stacks5", values, tab, n, n, True)
    assert same_bits(got, want), first_difference(got, want)
    es.close()


# ---- passes, output length -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dense8", "one_mod_two_carriers"])
def test_result_does_not_depend_on_the_pass_size(pkg, tab, name):
    n = 1024
    values = rows_of(GRAPHS[name][0])
    es = context(pkg, name, 10)
    for hop, glide in ((256, False), (131, True)):
        want = model(name, values, tab, n, hop, glide)
        assert len(want) > 2 * TILE  # several tiles and, below, several passes that end inside a tile
        for per_pass in (0, TILE - 1, TILE + 1):
            got = es.render_graph_continuous(values, hop, glide=glide, samples_per_pass=per_pass)
            assert same_bits(got, want), "hop %d samples_per_pass %d: %s" % (hop, per_pass, first_difference(got, want))
    es.close()


@pytest.mark.parametrize("hop", [1024, 101])
def test_output_shorter_and_longer_than_the_rendering(pkg, tab, hop):
    name, n, rows = "two_mods", 1024, 7
    values = rows_of(3)[:rows]
    covered = (rows - 1) * hop + n
    es = context(pkg, name, 10)
    for per_pass in (0, 1000):
        for length in (covered - 5, covered + 5, 3, 0):
            got = es.render_graph_continuous(values, hop, samples_per_pass=per_pass, out_samples=length)
            want = model(name, values, tab, n, hop, False, out_samples=length)
            assert got.shape == (length,)
            assert same_bits(got, want), first_difference(got, want)
        got = es.render_graph_continuous(values, hop, samples_per_pass=per_pass, out_samples=covered + 5)
        assert not bits(got[covered:]).any(), "the tail behind the rendering must be exactly +0"
    es.close()


# ---- the anchors on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("2op", 0), ("triple", 2)])
def test_anchor_graphs_equal_the_fixed_voices_renderer(pkg, name, kind):
    n, log2n = 1024, 10
    values = CM.track_rows(kind, 70, 100 * kind + 8)
    pmax4 = CM.PMAX[kind]
    pairs = GRAPHS[name][0] // 2
    fixed = pkg.HipES(32, 32, synth_kind=kind, audio_log2=log2n, param_max=pmax4, seed=SEED, workgroup_size=32)
    graph = context(pkg, name, log2n, ranges=([0.0] * (4 * pairs), pmax4 * pairs))
    for hop, glide in ((n, False), (256, True), (101, False), (1, True)):
        want = fixed.render_continuous(values, hop, glide=glide)
        got = graph.render_graph_continuous(values, hop, glide=glide)
        assert same_bits(got, want), "hop %d glide %d: %s" % (hop, glide, first_difference(got, want))
        assert np.abs(want).max() > 0.01
    fixed.close()
    graph.close()


# ---- context state ---------------------------------------------------------------------------------------------------------
def test_render_between_generations_leaves_the_run_alone(pkg, tab):
    name, log2n, n = "chain3", 10, 1024
    ranges = GM.audible_ranges(GRAPHS[name])
    values = rows_of(3)
    target = WM.graph_synth(GRAPHS[name], np.array([[0.4, 0.3, 0.2, 0.5, 0.1, 1.0]], np.float32), ranges[0], ranges[1], n, tab)[0]
    runs = []
    for render in (True, False):
        es = context(pkg, name, log2n, ranges=ranges, parents=512, offspring=1536)  # P = 2048: the selection with its lazy tail, splitters and lists
        es.track()
        es.set_target_audio(target)
        es.init_population(0)
        es.execute_generations(3)
        if render:
            es.render_graph_continuous(values, n // 4, glide=True, samples_per_pass=5000)
        assert es.generation == 3
        es.execute_generations(3)
        runs.append((es.read_population(), es.read_audio(), es.read_spectrum().view(np.float32), es.read_target(), es.best_ever(),
                     es.generation))
        es.close()
    (pa, aa, sa, ta, ba, ga), (pb, ab, sb, tb, bb, gb) = runs
    assert ga == gb == 6
    for what, x, y in zip(("values", "steps", "fitness"), pa, pb):
        assert same_bits(x, y), what
    assert same_bits(aa, ab) and same_bits(sa, sb) and same_bits(ta, tb)
    for x, y in zip(ba[:3], bb[:3]):
        assert same_bits(x, y)
    assert ba[3] == bb[3]


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(pkg, hip, tab):
    n, rows = 1024, 7
    INVALID, SIZE, STATE = -1, -4, -5
    L = hip.load()
    out = np.empty((rows - 1) * n + n, np.float32)

    def call(es, v, args, nbytes=None, num_rows=rows, output=out):
        return L.sots_render_graph_continuous(es._h, v.ctypes.data_as(C.c_void_p), v.nbytes if nbytes is None else nbytes, num_rows, args,
                                              output.ctypes.data_as(C.c_void_p) if output is not None else None, out.size)

    def args(hop=n, flags=0, per_pass=0, size=C.sizeof(hip.RenderContinuousArgs)):
        return C.byref(hip.RenderContinuousArgs(size, hop, flags, per_pass))

    # a context of a fixed voice
    fixed = pkg.HipES(32, 32, synth_kind=1, audio_log2=10, param_max=CM.PMAX[1], seed=SEED, workgroup_size=32)
    v6 = np.ascontiguousarray(CM.track_rows(1, rows, 108))
    assert call(fixed, v6, args()) == STATE
    assert b"sots_render_graph_continuous: the handle runs a fixed voice" in L.sots_last_error(fixed._h)
    with pytest.raises(pkg.SotsError) as e:
        fixed.render_graph_continuous(v6, n)
    assert e.value.code == STATE
    fixed.close()

    es = context(pkg, "chain3", 10)
    v = np.ascontiguousarray(rows_of(3)[:rows])
    assert call(es, v, args()) == 0
    want = out.copy()
    assert same_bits(want, model("chain3", v, tab, n, n, False))
    # feedback: refused while any index is not 0, rendered again once all are
    es.set_voice_feedback([0.0, 0.75, 0.0])
    assert call(es, v, args()) == STATE
    text = L.sots_last_error(es._h)
    assert b"sots_set_voice_feedback" in text and b"sots_render_overlap_add renders such a voice" in text and b"operator 1" in text
    es.set_voice_feedback([0.0, 0.0, 0.0])
    out[:] = 7.0
    assert call(es, v, args()) == 0 and same_bits(out, want)
    es.set_voice_feedback([2.0, 0.0, 0.0])
    assert call(es, v, args()) == STATE
    es.set_voice_feedback(None)
    assert call(es, v, args(flags=1)) == 0
    # the arguments
    assert call(es, v, None) == INVALID
    assert call(es, v, args(size=C.sizeof(hip.RenderContinuousArgs) - 4)) == INVALID
    assert call(es, v, args(hop=0)) == INVALID
    assert call(es, v, args(hop=n + 1)) == INVALID
    assert b"sots_render_graph_continuous: hop 1025 outside 1..1024" in L.sots_last_error(es._h)
    assert call(es, v, args(hop=1)) == 0
    assert call(es, v, args(flags=2)) == INVALID
    assert call(es, v, args(), nbytes=0, num_rows=0) == INVALID
    assert call(es, v, args(), nbytes=v.nbytes - 4) == SIZE
    assert b"values" in L.sots_last_error(es._h)
    assert call(es, v, args(hop=n), nbytes=(1 << 21) * 24, num_rows=1 << 21) == INVALID
    assert b"2^31" in L.sots_last_error(es._h)
    assert call(es, v, args(), output=None) == INVALID
    # ... and the fixed voices' renderer goes on refusing the graph voice
    assert L.sots_render_continuous(es._h, v.ctypes.data_as(C.c_void_p), v.nbytes, rows, args(), out.ctypes.data_as(C.c_void_p), out.size) == INVALID
    es.close()
