"""sots_render_graph_feedback against the per-sample loop of its NumPy statement,
tests/_render_graph_feedback_model.py, BIT FOR BIT and with no tolerance, in both forms of the chain: the phases are sums of
32-bit integers, the chain over the samples has exactly one solution, and everything else is per-sample fp32 with one rounding
per operation.  tests/test_render_graph_feedback_cpu.py asserts on the model what the cases used here cover
(tests/_render_graph_feedback_cases.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _graph_waveforms_model as WM  # noqa: E402
import _render_continuous_model as CM  # noqa: E402
import _render_graph_continuous_model as GM  # noqa: E402
import _render_graph_feedback_model as RM  # noqa: E402
from _render_graph_feedback_cases import BASE, BASE_IDS, BASE_SHAPE, CHAIN3_CARRY, SHARED, mixed_level_cases, waveform_case  # noqa: E402

pytestmark = pytest.mark.gpu

GRAPHS = GM.GRAPHS
SEED = 0x5EED0001
SERIAL, RELAX = 1, 2
FORMS = [SERIAL, RELAX]
bits = RM.bits


def first_difference(got, want):
    if got.shape != want.shape:
        return "shapes %r and %r" % (got.shape, want.shape)
    d = np.flatnonzero(bits(got) != bits(want))
    return "equal" if d.size == 0 else "%d samples differ, first at %d: got %r want %r" % (d.size, d[0], got[d[0]], want[d[0]])


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


@pytest.fixture(scope="module")
def tab(O):
    return O.wavetable()


def rows_of(ops, rows=7):
    return GM.graph_rows(ops, rows, 100 + ops)


def context(pkg, name, log2n, ranges=None, waves=None, beta=None, parents=32, offspring=32):
    pmin, pmax = ranges or WM.ranges(GRAPHS[name][0])
    es = pkg.HipES(parents, offspring, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=log2n, param_min=pmin, param_max=pmax, seed=SEED,
                   workgroup_size=32, graph=pkg.capi.make_voice_graph(*GRAPHS[name]), waveforms=waves)
    if beta is not None:
        es.set_voice_feedback(beta)
    return es


_MODEL = {}


def model(name, waves, beta, rows, tab, n, hop, glide, ranges=None, out_samples=None):
    """the loop model's rendering, made once per case and left unchanged"""
    key = (name, tuple(waves or ()), tuple(beta or ()), rows, n, hop, glide, out_samples, ranges is not None)
    if key not in _MODEL:
        ops = GRAPHS[name][0]
        pmin, pmax = ranges or WM.ranges(ops)
        _MODEL[key] = RM.render(GRAPHS[name], waves, beta, rows_of(ops, rows), pmin, pmax, tab, n, hop, glide, out_samples=out_samples)
        _MODEL[key].setflags(write=False)
    return _MODEL[key]


# ---- the base shape: device == model, both forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", BASE, ids=BASE_IDS)
def test_base_cases_equal_the_model(pkg, tab, case, form):
    name, waves, beta = case
    n, rows, hop = BASE_SHAPE
    es = context(pkg, name, 8, waves=waves, beta=beta)
    values = rows_of(GRAPHS[name][0], rows)
    for glide in (False, True):
        got = es.render_graph_feedback(values, hop, glide=glide, chain_form=form)
        want = model(name, waves, beta, rows, tab, n, hop, glide)
        assert got.shape == (862,)
        assert same_bits(got, want), "glide %d: %s" % (glide, first_difference(got, want))
        assert np.abs(want).max() > 0.01
    es.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("w", list(WM.WAVES))
def test_every_waveform_on_a_feedback_modulator_and_carrier(pkg, tab, w, form):
    name, waves, beta = waveform_case(w)
    n, rows, hop = BASE_SHAPE
    es = context(pkg, name, 8, waves=waves, beta=beta)
    for glide in (False, True):
        got = es.render_graph_feedback(rows_of(3, rows), hop, glide=glide, chain_form=form)
        want = model(name, waves, beta, rows, tab, n, hop, glide)
        assert same_bits(got, want), "glide %d: %s" % (glide, first_difference(got, want))
    es.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("b", [2.0, 1e-10])
def test_beta_extremes(pkg, tab, b, form):
    n, rows, hop = BASE_SHAPE
    beta = [b, b, b]
    es = context(pkg, "chain3", 8, beta=beta)
    got = es.render_graph_feedback(rows_of(3, rows), hop, glide=True, chain_form=form)
    want = model("chain3", None, beta, rows, tab, n, hop, True)
    assert same_bits(got, want), first_difference(got, want)
    if b < 1.0:  # an index that is not 0 goes through the chain, and its offset always fixes to 0: the rendering of 4.16
        es.set_voice_feedback(None)
        assert same_bits(got, es.render_graph_continuous(rows_of(3, rows), hop, glide=True))
    es.close()


@pytest.mark.parametrize("cap", [8, 4096])
def test_relaxation_caps(pkg, tab, cap):
    """cap 8: every case's tile is finished serially from sample 8 on (asserted on the model); cap 4096: never"""
    n, rows, hop = BASE_SHAPE
    for name, waves, beta in (BASE[2], BASE[5]):
        es = context(pkg, name, 8, waves=waves, beta=beta)
        got = es.render_graph_feedback(rows_of(GRAPHS[name][0], rows), hop, chain_form=RELAX, relax_cap=cap)
        want = model(name, waves, beta, rows, tab, n, hop, False)
        assert same_bits(got, want), "%s: %s" % (name, first_difference(got, want))
        es.close()


# ---- several tiles, passes, lengths ---------------------------------------------------------------------------------------------
def test_several_tiles_with_a_carry(pkg, tab):
    name, waves, beta, rows, n, hop = CHAIN3_CARRY
    es = context(pkg, name, 8, beta=beta)
    want = model(name, waves, beta, rows, tab, n, hop, True)
    assert len(want) == 17920
    for form, cap in ((SERIAL, 0), (RELAX, 0), (RELAX, 8), (0, 0)):
        got = es.render_graph_feedback(rows_of(3, rows), hop, glide=True, chain_form=form, relax_cap=cap)
        assert same_bits(got, want), "form %d cap %d: %s" % (form, cap, first_difference(got, want))
    es.close()


@pytest.mark.parametrize("form", FORMS)
def test_result_does_not_depend_on_the_pass_size(pkg, tab, form):
    """h1 and h2 are carried beside the end phases; passes that end inside a tile, and passes of one sample"""
    name, waves, beta, rows, n, hop = CHAIN3_CARRY
    es = context(pkg, name, 8, beta=beta)
    want = model(name, waves, beta, rows, tab, n, hop, False)
    for per_pass in (4095, 4097):
        got = es.render_graph_feedback(rows_of(3, rows), hop, samples_per_pass=per_pass, chain_form=form)
        assert same_bits(got, want), "samples_per_pass %d: %s" % (per_pass, first_difference(got, want))
    got = es.render_graph_feedback(rows_of(3, rows), hop, samples_per_pass=1, chain_form=form, out_samples=300)
    assert same_bits(got, want[:300]), first_difference(got, want[:300])
    es.close()


def test_output_shorter_and_longer_than_the_rendering(pkg, tab):
    name, waves, beta = BASE[2]
    n, rows, hop = BASE_SHAPE
    es = context(pkg, name, 8, beta=beta)
    want = model(name, waves, beta, rows, tab, n, hop, False)
    covered = len(want)
    for form in FORMS:
        for per_pass in (0, 500):
            for length in (covered - 5, covered + 5, 3, 0):
                got = es.render_graph_feedback(rows_of(3, rows), hop, samples_per_pass=per_pass, chain_form=form, out_samples=length)
                assert got.shape == (length,)
                assert same_bits(got[:covered], want[:length]), first_difference(got[:covered], want[:length])
                assert not bits(got[covered:]).any(), "the tail behind the rendering must be exactly +0"
    es.close()


# ---- anchors and state ------------------------------------------------------------------------------------------------------------
def test_without_feedback_it_is_sots_render_graph_continuous(pkg, tab):
    n, rows, hop = BASE_SHAPE
    es = context(pkg, "dense8", 8, waves=GM.MIXED8)
    values = rows_of(8, rows)
    for glide in (False, True):
        want = es.render_graph_continuous(values, hop, glide=glide)
        for form in (0, SERIAL, RELAX):
            got = es.render_graph_feedback(values, hop, glide=glide, chain_form=form)
            assert same_bits(got, want), "glide %d form %d: %s" % (glide, form, first_difference(got, want))
    es.close()


def test_scratch_of_a_feedback_rendering_is_not_read_without_feedback(pkg, tab):
    """the t buffer and h1, h2 that a rendering with feedback left behind, under an empty mask"""
    name, n, hop, rows, per_pass = SHARED
    beta = [0.0, 1.0, 0.0]
    es = context(pkg, name, 8, beta=beta)
    values = rows_of(3, rows)
    got = es.render_graph_feedback(values, hop, samples_per_pass=per_pass)
    want = model(name, None, beta, rows, tab, n, hop, False)
    assert len(want) == 5312 and same_bits(got, want), first_difference(got, want)
    es.set_voice_feedback(None)
    pmin, pmax = WM.ranges(3)
    plain = GM.render(GRAPHS[name], None, values, pmin, pmax, tab, n, hop)
    assert not same_bits(plain, want)
    old = es.render_graph_continuous(values, hop, samples_per_pass=per_pass)
    new = es.render_graph_feedback(values, hop, samples_per_pass=per_pass)
    assert same_bits(old, plain), first_difference(old, plain)
    assert same_bits(new, plain), first_difference(new, plain)
    assert same_bits(old, new)
    es.close()


def test_a_rendering_without_feedback_leaves_nothing_for_one_with(pkg, tab):
    """h1 and h2 start from +0 although the call before cleared only the phases, and again after a chain has left its own"""
    name, n, hop, rows, per_pass = SHARED
    beta = [0.0, 0.0, 0.5]
    es = context(pkg, name, 8)
    values = rows_of(3, rows)
    es.render_graph_continuous(values, hop, samples_per_pass=per_pass)
    es.set_voice_feedback(beta)
    want = model(name, None, beta, rows, tab, n, hop, False)
    for form in FORMS:
        got = es.render_graph_feedback(values, hop, samples_per_pass=per_pass, chain_form=form)
        assert same_bits(got, want), "form %d: %s" % (form, first_difference(got, want))
    es.close()


@pytest.mark.parametrize("case", mixed_level_cases(), ids=["square-flagged", "sine-flagged"])
def test_a_level_with_a_flagged_and_an_unflagged_modulator(pkg, tab, case):
    name, waves, beta = case
    n, rows, hop = BASE_SHAPE
    es = context(pkg, name, 8, waves=waves, beta=beta)
    for glide in (False, True):
        got = es.render_graph_feedback(rows_of(8, rows), hop, glide=glide)
        want = model(name, waves, beta, rows, tab, n, hop, glide)
        assert same_bits(got, want), "glide %d: %s" % (glide, first_difference(got, want))
        assert np.abs(want).max() > 0.01
    es.close()


def test_the_old_entry_point_still_refuses_feedback(pkg):
    es = context(pkg, "chain3", 8, beta=[0.0, 0.5, 0.0])
    with pytest.raises(pkg.SotsError) as e:
        es.render_graph_continuous(rows_of(3), 101)
    assert e.value.code == -5 and "sots_render_overlap_add renders such a voice" in str(e.value)
    assert es.render_graph_feedback(rows_of(3), 101).shape == (862,)
    es.close()


def test_render_between_generations_leaves_the_run_alone(pkg, tab):
    name, log2n, n = "chain3", 10, 1024
    ranges = GM.audible_ranges(GRAPHS[name])
    values = rows_of(3, 70)
    target = WM.graph_synth(GRAPHS[name], np.array([[0.4, 0.3, 0.2, 0.5, 0.1, 1.0]], np.float32), ranges[0], ranges[1], n, tab)[0]
    runs = []
    for render in (True, False):
        es = context(pkg, name, log2n, ranges=ranges, beta=[0.0, 0.5, 0.75], parents=512, offspring=1536)  # P = 2048
        es.track()
        es.set_target_audio(target)
        es.init_population(0)
        es.execute_generations(3)
        if render:
            es.render_graph_feedback(values, n // 4, glide=True, samples_per_pass=5000, chain_form=RELAX)
            es.render_graph_feedback(values[:7], n // 4, chain_form=SERIAL)
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
    A = hip.RenderGraphFeedbackArgs

    def call(es, v, args, nbytes=None, num_rows=rows, output=out):
        return L.sots_render_graph_feedback(es._h, v.ctypes.data_as(C.c_void_p), v.nbytes if nbytes is None else nbytes, num_rows, args,
                                            output.ctypes.data_as(C.c_void_p) if output is not None else None, out.size)

    def args(hop=n, flags=0, per_pass=0, form=0, cap=0, size=C.sizeof(A)):
        return C.byref(A(size, hop, flags, per_pass, form, cap))

    # a context of a fixed voice
    fixed = pkg.HipES(32, 32, synth_kind=1, audio_log2=10, param_max=CM.PMAX[1], seed=SEED, workgroup_size=32)
    v6 = np.ascontiguousarray(CM.track_rows(1, rows, 108))
    assert call(fixed, v6, args()) == STATE
    assert b"sots_render_graph_feedback: the handle runs a fixed voice" in L.sots_last_error(fixed._h)
    with pytest.raises(pkg.SotsError) as e:
        fixed.render_graph_feedback(v6, n)
    assert e.value.code == STATE
    fixed.close()

    beta = [0.0, 0.75, 0.0]
    es = context(pkg, "chain3", 10, beta=beta)
    v = np.ascontiguousarray(rows_of(3, rows))
    assert call(es, v, args()) == 0
    pmin, pmax = WM.ranges(3)
    assert same_bits(out, RM.render(GRAPHS["chain3"], None, beta, v, pmin, pmax, tab, n, n, form="relax"))
    assert call(es, v, args(flags=1, form=2, cap=4096)) == 0
    # the arguments
    assert call(es, v, None) == INVALID
    assert call(es, v, args(size=C.sizeof(A) - 4)) == INVALID
    assert call(es, v, args(size=C.sizeof(hip.RenderContinuousArgs))) == INVALID
    assert call(es, v, args(hop=0)) == INVALID
    assert call(es, v, args(hop=n + 1)) == INVALID
    assert b"sots_render_graph_feedback: hop 1025 outside 1..1024" in L.sots_last_error(es._h)
    assert call(es, v, args(flags=2)) == INVALID
    assert call(es, v, args(form=3)) == INVALID
    assert b"chain_form 3" in L.sots_last_error(es._h)
    assert call(es, v, args(form=2, cap=4097)) == INVALID
    assert b"relax_cap 4097" in L.sots_last_error(es._h)
    assert call(es, v, args(), nbytes=0, num_rows=0) == INVALID
    assert call(es, v, args(), nbytes=v.nbytes - 4) == SIZE
    assert b"values" in L.sots_last_error(es._h)
    assert call(es, v, args(hop=n), nbytes=(1 << 21) * 24, num_rows=1 << 21) == INVALID
    assert b"2^31" in L.sots_last_error(es._h)
    assert call(es, v, args(), output=None) == INVALID
    es.close()
