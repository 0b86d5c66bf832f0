"""sots_render_graph_genes against the per-sample loop of its NumPy statement,
tests/_render_graph_genes_model.py, BIT FOR BIT and with no tolerance, in both forms of the chain: the phases are sums of 32-bit
integers, the chain over the samples has exactly one solution whether B is a constant or a value per sample, and everything
else is per-sample fp32 with one rounding per operation.  tests/test_render_graph_genes_cpu.py asserts on the model what the
cases used here cover (tests/_render_graph_genes_cases.py): every branch of the effective index, tiles that hit a cap of 8
and tiles that settle before it."""
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
import _render_graph_genes_model as NM  # noqa: E402
from _render_graph_genes_cases import CASES, GRAPHS, N, SHAPES, finite_rows, fixed_twin, ranges, rows_of, waveform_case  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x5EED0001
LIBRARY, SERIAL, RELAX = 0, 1, 2
FORMS = [LIBRARY, SERIAL, RELAX]
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


def context(pkg, case, log2n=8, rng=None, mask=None, beta=None, parents=32, offspring=32):
    """a context of the case's voice; mask and beta replace the case's (a mask of 0: sots_create_graph)"""
    name, waves, case_beta, case_mask = case
    mask = case_mask if mask is None else mask
    pmin, pmax = rng or ranges(case)
    kw = dict(feedback_genes=mask) if mask else {}
    es = pkg.HipES(parents, offspring, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=log2n, param_min=pmin, param_max=pmax, seed=SEED,
                   workgroup_size=32, graph=pkg.capi.make_voice_graph(*GRAPHS[name]), waveforms=waves, **kw)
    beta = case_beta if beta is None else beta
    if any(beta):
        es.set_voice_feedback(beta)
    return es


_MODEL = {}


def model(tab, key, case, shape, glide):
    """the loop model's rendering, made once per case and left unchanged"""
    if (key, shape, glide) not in _MODEL:
        name, waves, beta, mask = case
        rows, hop = SHAPES[shape]
        pmin, pmax = ranges(case)
        _MODEL[(key, shape, glide)] = NM.render(GRAPHS[name], waves, beta, mask, rows_of(case, rows), pmin, pmax, tab, N, hop, glide)
        _MODEL[(key, shape, glide)].setflags(write=False)
    return _MODEL[(key, shape, glide)]


# ---- device == model: the cases, every form -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS, ids=["library", "serial", "relax"])
@pytest.mark.parametrize("key", list(CASES))
def test_cases_equal_the_model(pkg, tab, key, form):
    """the carrier's gene (D = 5), a gene operator beside one of a fixed index (D = 7), five gene operators (D = 15); rows that
    hold 0, 1, values between and beyond, NaN and both infinities"""
    case = CASES[key]
    es = context(pkg, case)
    values = rows_of(case, 7)
    for glide in (False, True):
        got = es.render_graph_genes(values, 101, glide=glide, chain_form=form)
        want = model(tab, key, case, "7x101", glide)
        assert got.shape == (862,)
        assert same_bits(got, want), "glide %d: %s" % (glide, first_difference(got, want))
        assert np.abs(want).max() > 0.01
    es.close()


@pytest.mark.parametrize("form", [SERIAL, RELAX], ids=["serial", "relax"])
@pytest.mark.parametrize("w", list(WM.WAVES))
def test_every_waveform_on_a_gene_modulator_and_carrier(pkg, tab, w, form):
    case = waveform_case(w)
    es = context(pkg, case)
    for glide in (False, True):
        got = es.render_graph_genes(rows_of(case, 7), 101, glide=glide, chain_form=form)
        want = model(tab, ("wave", w), case, "7x101", glide)
        assert same_bits(got, want), "glide %d: %s" % (glide, first_difference(got, want))
    es.close()


@pytest.mark.parametrize("cap", [8, 4096])
@pytest.mark.parametrize("key", list(CASES))
def test_relaxation_caps(pkg, tab, key, cap):
    """cap 8 on the 70-row track: tiles that are finished in order from sample 8 on, with B out of LDS, beside tiles that
    settle at the first sweep (asserted on the model); cap 4096: never hit"""
    case = CASES[key]
    es = context(pkg, case)
    for shape in ("7x101", "70x101"):
        rows, hop = SHAPES[shape]
        got = es.render_graph_genes(rows_of(case, rows), hop, glide=True, chain_form=RELAX, relax_cap=cap)
        want = model(tab, key, case, shape, True)
        assert same_bits(got, want), "%s: %s" % (shape, first_difference(got, want))
    es.close()


@pytest.mark.parametrize("shape", ["7x1", "7xN"])
def test_a_row_per_sample_and_rows_that_do_not_overlap(pkg, tab, shape):
    case = CASES["chain3_gene_beside_fixed"]
    es = context(pkg, case)
    rows, hop = SHAPES[shape]
    for glide in (False, True):
        for form in (SERIAL, RELAX):
            got = es.render_graph_genes(rows_of(case, rows), hop, glide=glide, chain_form=form)
            want = model(tab, "chain3_gene_beside_fixed", case, shape, glide)
            assert same_bits(got, want), "glide %d form %d: %s" % (glide, form, first_difference(got, want))
    es.close()


# ---- several tiles, passes, lengths ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [SERIAL, RELAX], ids=["serial", "relax"])
@pytest.mark.parametrize("key", list(CASES))
def test_result_does_not_depend_on_the_pass_size(pkg, tab, key, form):
    """7225 samples: passes that end one sample before and one behind a tile of the scans, so that a pass takes h1, h2 and its
    rows' B where the pass before left off"""
    case = CASES[key]
    es = context(pkg, case)
    rows, hop = SHAPES["70x101"]
    values = rows_of(case, rows)
    for glide in (False, True):
        want = model(tab, key, case, "70x101", glide)
        assert len(want) == 7225
        for per_pass in (0, 4095, 4097):
            got = es.render_graph_genes(values, hop, glide=glide, samples_per_pass=per_pass, chain_form=form)
            assert same_bits(got, want), "glide %d samples_per_pass %d: %s" % (glide, per_pass, first_difference(got, want))
    es.close()


@pytest.mark.parametrize("form", [SERIAL, RELAX], ids=["serial", "relax"])
def test_passes_of_one_sample(pkg, tab, form):
    case = CASES["2op_carrier"]
    es = context(pkg, case)
    rows, hop = SHAPES["70x101"]
    want = model(tab, "2op_carrier", case, "70x101", True)
    got = es.render_graph_genes(rows_of(case, rows), hop, glide=True, samples_per_pass=1, chain_form=form)
    assert same_bits(got, want), first_difference(got, want)
    es.close()


def test_output_shorter_and_longer_than_the_rendering(pkg, tab):
    case = CASES["chain3_gene_beside_fixed"]
    es = context(pkg, case)
    want = model(tab, "chain3_gene_beside_fixed", case, "7x101", False)
    covered = len(want)
    for form in (SERIAL, RELAX):
        for per_pass in (0, 500):
            for length in (covered - 5, covered + 5, 3, 0):
                got = es.render_graph_genes(rows_of(case, 7), 101, samples_per_pass=per_pass, chain_form=form, out_samples=length)
                assert got.shape == (length,)
                assert same_bits(got[:covered], want[:length]), first_difference(got[:covered], want[:length])
                assert not bits(got[covered:]).any(), "the tail behind the rendering must be exactly +0"
    es.close()


# ---- anchors and state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [None, [0.5, 0.0, 2.0]], ids=["no-feedback", "feedback"])
def test_with_a_mask_of_0_it_is_sots_render_graph_feedback(pkg, tab, beta):
    """anchor (a), byte for byte, whatever the form and the pass size"""
    case = ("chain3", [0, 3, 6], beta or [0.0] * 3, 0)
    es = context(pkg, case, rng=WM.ranges(3))
    values = GM.graph_rows(3, 70, 103)
    for glide in (False, True):
        for form, cap, per_pass in ((LIBRARY, 0, 0), (SERIAL, 0, 4097), (RELAX, 8, 0)):
            want = es.render_graph_feedback(values, 101, glide=glide, chain_form=form, relax_cap=cap, samples_per_pass=per_pass)
            got = es.render_graph_genes(values, 101, glide=glide, chain_form=form, relax_cap=cap, samples_per_pass=per_pass)
            assert got.tobytes() == want.tobytes(), "glide %d form %d: %s" % (glide, form, first_difference(got, want))
    if beta is None:
        assert same_bits(es.render_graph_genes(values, 101), es.render_graph_continuous(values, 101))
    es.close()


@pytest.mark.parametrize("b", [0.0, 0.25, 1.0, 2.0])
@pytest.mark.parametrize("key", list(CASES))
def test_a_constant_index_is_a_context_of_the_fixed_setting(pkg, tab, key, b):
    """anchor (b): a gene range [b, b] and any finite gene against sots_render_graph_feedback on a second context with the
    index b set on those operators, fed the same rows without their gene columns"""
    case = CASES[key]
    rows = finite_rows(case, 70)
    pmin, pmax = ranges(case, b, b)
    beta, cols = fixed_twin(case, b)
    gene = context(pkg, case, rng=(pmin, pmax))
    fixed = context(pkg, case, rng=(pmin[cols], pmax[cols]), mask=0, beta=beta)
    assert gene.D == rows.shape[1] and fixed.D == cols.stop
    for glide in (False, True):
        for form in (SERIAL, RELAX):
            want = fixed.render_graph_feedback(np.ascontiguousarray(rows[:, cols]), 101, glide=glide, chain_form=form)
            got = gene.render_graph_genes(rows, 101, glide=glide, chain_form=form)
            assert got.tobytes() == want.tobytes(), "glide %d form %d: %s" % (glide, form, first_difference(got, want))
    gene.close()
    fixed.close()


def test_a_rendering_starts_from_nothing_that_the_one_before_left(pkg, tab):
    """h1, h2, the t buffers and the gene columns of another track stay in the context's scratch: none of it is read"""
    case = CASES["chain3_gene_beside_fixed"]
    es = context(pkg, case)
    es.render_graph_genes(rows_of(case, 70), 101, glide=True, chain_form=RELAX)
    for form in (SERIAL, RELAX):
        got = es.render_graph_genes(rows_of(case, 7), 101, chain_form=form)
        want = model(tab, "chain3_gene_beside_fixed", case, "7x101", False)
        assert same_bits(got, want), "form %d: %s" % (form, first_difference(got, want))
    es.close()


def test_render_between_generations_leaves_the_run_alone(pkg, tab):
    case = CASES["chain3_gene_beside_fixed"]
    name, log2n, n = case[0], 10, 1024
    pmin, pmax = GM.audible_ranges(GRAPHS[name])
    rng = (pmin + [0.0], pmax + [2.0])
    values = rows_of(case, 70)
    target = WM.graph_synth(GRAPHS[name], np.array([[0.4, 0.3, 0.2, 0.5, 0.1, 1.0]], np.float32), pmin, pmax, n, tab)[0]
    runs = []
    for render in (True, False):
        es = context(pkg, case, log2n=log2n, rng=rng, parents=512, offspring=1536)  # P = 2048
        es.track()
        es.set_target_audio(target)
        es.init_population(0)
        es.execute_generations(3)
        if render:
            es.render_graph_genes(values, n // 4, glide=True, samples_per_pass=5000, chain_form=RELAX)
            es.render_graph_genes(values[:7], n // 4, chain_form=SERIAL)
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
def test_the_entry_points_of_the_fixed_setting_still_refuse_a_gene_context(pkg):
    case = CASES["chain3_gene_beside_fixed"]
    es = context(pkg, case)
    values = rows_of(case, 7)
    for call, who in ((es.render_graph_continuous, "sots_render_graph_continuous"), (es.render_graph_feedback, "sots_render_graph_feedback")):
        with pytest.raises(pkg.SotsError) as e:
            call(values, 101)
        assert e.value.code == -5
        assert (who + ": the feedback indices of operators 0x2 are genes (sots_create_graph_genes): every row has its own; "
                "sots_render_overlap_add renders such a voice") in str(e.value)
    assert es.render_graph_genes(values, 101).shape == (862,)
    es.close()


def test_refusals_through_the_c_abi(pkg, hip, tab):
    n, rows = 1024, 7
    INVALID, SIZE, STATE = -1, -4, -5
    L = hip.load()
    out = np.empty((rows - 1) * n + n, np.float32)
    A = hip.RenderGraphFeedbackArgs

    def call(es, v, args, nbytes=None, num_rows=rows, output=out):
        return L.sots_render_graph_genes(es._h, v.ctypes.data_as(C.c_void_p), v.nbytes if nbytes is None else nbytes, num_rows, args,
                                         output.ctypes.data_as(C.c_void_p) if output is not None else None, out.size)

    def args(hop=n, flags=0, per_pass=0, form=0, cap=0, size=C.sizeof(A)):
        return C.byref(A(size, hop, flags, per_pass, form, cap))

    # a context of a fixed voice
    fixed = pkg.HipES(32, 32, synth_kind=1, audio_log2=10, param_max=CM.PMAX[1], seed=SEED, workgroup_size=32)
    v6 = np.ascontiguousarray(CM.track_rows(1, rows, 108))
    assert call(fixed, v6, args()) == STATE
    assert b"sots_render_graph_genes: the handle runs a fixed voice" in L.sots_last_error(fixed._h)
    with pytest.raises(pkg.SotsError) as e:
        fixed.render_graph_genes(v6, n)
    assert e.value.code == STATE
    fixed.close()

    case = CASES["chain3_gene_beside_fixed"]
    es = context(pkg, case, log2n=10)
    v = np.ascontiguousarray(rows_of(case, rows))
    assert es.D == 7 and v.shape == (rows, 7)
    assert call(es, v, args()) == 0
    pmin, pmax = ranges(case)
    assert same_bits(out, NM.render(GRAPHS["chain3"], None, case[2], case[3], v, pmin, pmax, tab, n, n, form="relax"))
    assert call(es, v, args(flags=1, form=2, cap=4096)) == 0
    # the arguments
    assert call(es, v, None) == INVALID
    assert call(es, v, args(size=C.sizeof(A) - 4)) == INVALID
    assert call(es, v, args(size=C.sizeof(hip.RenderContinuousArgs))) == INVALID
    assert call(es, v, args(hop=0)) == INVALID
    assert call(es, v, args(hop=n + 1)) == INVALID
    assert b"sots_render_graph_genes: hop 1025 outside 1..1024" in L.sots_last_error(es._h)
    assert call(es, v, args(flags=2)) == INVALID
    assert call(es, v, args(form=3)) == INVALID
    assert b"sots_render_graph_genes: chain_form 3" in L.sots_last_error(es._h)
    assert call(es, v, args(form=2, cap=4097)) == INVALID
    assert b"sots_render_graph_genes: relax_cap 4097" in L.sots_last_error(es._h)
    assert call(es, v, args(), nbytes=0, num_rows=0) == INVALID
    assert call(es, v, args(), nbytes=v.nbytes - 4) == SIZE
    assert b"values" in L.sots_last_error(es._h)
    assert call(es, v, args(), nbytes=rows * 6 * 4) == SIZE  # rows of 2 OPS genes: the context's D counts the gene column
    assert b"7 rows need 196 bytes of values, got 168" in L.sots_last_error(es._h)
    assert call(es, v, args(hop=n), nbytes=(1 << 21) * 28, num_rows=1 << 21) == INVALID
    assert b"2^31" in L.sots_last_error(es._h)
    assert call(es, v, args(), output=None) == INVALID
    es.close()
