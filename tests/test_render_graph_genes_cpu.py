"""CPU checks of the phase-continuous rendering of a graph voice whose feedback indices are genes (sots_render_graph_genes,
DESIGN.md 4.19): the NumPy model's two statements of the chain against each other with B a value per sample, what the rows of
the cases cover, the anchors in the models of the fixed setting, pass sizes and output lengths, the rules under sanitizers, the
library's export, the call without a handle and the renderMode names of the host layer.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _graph_waveforms_model as WM  # noqa: E402
import _render_graph_continuous_model as GM  # noqa: E402
import _render_graph_feedback_model as RM  # noqa: E402
import _render_graph_genes_model as NM  # noqa: E402
from _graph_voice_match import CHAIN3, NO_DEVICE, PMAX3, run_match  # noqa: E402
from _render_graph_genes_cases import CASES, GRAPHS, N, SHAPES, finite_rows, fixed_twin, ranges, rows_of, waveform_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
HOST = os.path.join(PKG_DIR, "host")
bits = RM.bits


@pytest.fixture(scope="module")
def tab(O):
    return O.wavetable()


def render(tab, case, shape, glide, rows=None, rng=None, **kw):
    name, waves, beta, mask = case
    count, hop = SHAPES[shape]
    pmin, pmax = rng or ranges(case)
    return NM.render(GRAPHS[name], waves, beta, mask, rows_of(case, count) if rows is None else rows, pmin, pmax, tab, N, hop, glide, **kw)


_LOOPS = {}


def loop_of(tab, key, case, shape, glide):
    """the loop form's rendering, made once per case and left unchanged"""
    if (key, shape, glide) not in _LOOPS:
        _LOOPS[(key, shape, glide)] = render(tab, case, shape, glide)
        _LOOPS[(key, shape, glide)].setflags(write=False)
    return _LOOPS[(key, shape, glide)]


# ---- the two statements of the chain ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("glide", [False, True], ids=["hold", "glide"])
@pytest.mark.parametrize("cap", [8, 4096])
@pytest.mark.parametrize("tile", [256, 1024])
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("key", list(CASES))
def test_loop_and_relaxation_agree_bit_for_bit(tab, key, shape, tile, cap, glide):
    case = CASES[key]
    sweeps = []
    got = render(tab, case, shape, glide, form="relax", tile=tile, cap=cap, sweeps=sweeps)
    want = loop_of(tab, key, case, shape, glide)
    count, hop = SHAPES[shape]
    assert len(want) == (count - 1) * hop + N
    assert np.array_equal(bits(got), bits(want))
    assert np.abs(want).max() > 0.01
    flagged = bin(case[3]).count("1") + sum(1 for b in case[2] if b)
    assert len(sweeps) == flagged * -(-len(want) // tile) and all(1 <= s <= min(cap, tile) for _, s, _ in sweeps)


@pytest.mark.parametrize("glide", [False, True], ids=["hold", "glide"])
@pytest.mark.parametrize("cap", [8, 4096])
@pytest.mark.parametrize("w", list(WM.WAVES))
def test_every_waveform_on_a_gene_operator(tab, w, cap, glide):
    case = waveform_case(w)
    got = render(tab, case, "7x101", glide, form="relax", tile=1024, cap=cap)
    assert np.array_equal(bits(got), bits(loop_of(tab, ("wave", w), case, "7x101", glide)))


# ---- what the rows cover ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_the_rows_reach_every_branch_of_the_effective_index_and_both_its_bounds(tab, key):
    case = CASES[key]
    name, _, _, mask = case
    ops = GRAPHS[name][0]
    g = rows_of(case)[:, 2 * ops:]
    flat = g.ravel()  # the 7-row track's gene columns: 0, 1, between, -0.5, 1.5, NaN, +inf and, with a second column, -inf
    assert np.isnan(flat).any() and (flat == np.inf).any() and (flat == 0).any() and (flat == 1).any() and (flat == -0.5).any() and (flat == 1.5).any()
    if g.shape[1] > 1:
        assert (flat == -np.inf).any()
    for glide in (False, True):
        betas = {}
        render(tab, case, "7x101", glide, form="relax", betas=betas)
        assert sorted(betas) == [j for j in range(ops) if mask >> j & 1]
        for j, per_pass in betas.items():
            b = np.concatenate(per_pass)
            assert not np.isnan(b).any() and b.min() == 0.0 and b.max() == 2.0, (j, glide)
            assert not np.signbit(b[b == 0]).any(), "the effective index is +0, never -0"
        b = np.concatenate([x for per_pass in betas.values() for x in per_pass])
        assert ((b > 0) & (b < 2)).any(), glide


@pytest.mark.parametrize("key", list(CASES))
def test_with_a_cap_of_8_some_tile_hits_the_cap_and_some_tile_settles_before_it(tab, key):
    """on the device's tile of 1024 samples, in the 70-row track, whose rows 18 .. 32 are quiet; and with tiles of 256 in the
    7-row track, whose first two rows are quiet in the first gene column"""
    case = CASES[key]
    for shape, tile in (("70x101", 1024), ("7x101", 256)):
        for glide in (False, True):
            sweeps = []
            render(tab, case, shape, glide, form="relax", tile=tile, cap=8, sweeps=sweeps)
            gene = [(s, c) for j, s, c in sweeps if case[3] >> j & 1]
            assert any(c for _, c in gene), (shape, glide)
            assert any(not c and s < 8 for s, c in gene), (shape, glide)
            assert any(not c and s == 1 for s, c in gene), "a quiet tile is its own first guess"


def test_a_cap_of_4096_is_never_hit(tab):
    sweeps = []
    render(tab, CASES["2op_carrier"], "70x101", True, form="relax", tile=1024, cap=4096, sweeps=sweeps)
    assert len(sweeps) == 8 and not any(c for _, _, c in sweeps)


# ---- anchors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("glide", [False, True], ids=["hold", "glide"])
@pytest.mark.parametrize("b", [0.0, 0.25, 1.0, 2.0])
@pytest.mark.parametrize("key", list(CASES))
def test_a_constant_index_is_the_fixed_setting(tab, key, b, glide):
    """anchor (b): a gene range [b, b] and any finite gene"""
    case = CASES[key]
    name, waves, _, _ = case
    rows = finite_rows(case)
    pmin, pmax = ranges(case, b, b)
    beta, cols = fixed_twin(case, b)
    ops = GRAPHS[name][0]
    want = RM.render(GRAPHS[name], waves, beta, rows[:, cols], pmin[:2 * ops], pmax[:2 * ops], tab, N, 101, glide)
    for form in ("loop", "relax"):
        got = render(tab, case, "7x101", glide, rows=rows, rng=(pmin, pmax), form=form)
        assert np.array_equal(bits(got), bits(want)), form
    if b == 0.0 and not any(case[2]):  # the chain with an index of +0 is the voice without feedback
        plain = GM.render(GRAPHS[name], waves, rows[:, cols], pmin[:2 * ops], pmax[:2 * ops], tab, N, 101, glide)
        assert np.array_equal(bits(plain), bits(want))


def test_with_a_mask_of_0_it_is_the_model_of_the_fixed_setting(tab):
    """anchor (a) on the models"""
    pmin, pmax = WM.ranges(3)
    rows = GM.graph_rows(3, 7, 103)
    beta = [0.5, 0.0, 1.0]
    want = RM.render(GRAPHS["chain3"], [0, 3, 0], beta, rows, pmin, pmax, tab, N, 101, True)
    got = NM.render(GRAPHS["chain3"], [0, 3, 0], beta, 0, rows, pmin, pmax, tab, N, 101, True, form="relax")
    assert np.array_equal(bits(got), bits(want))


# ---- passes and lengths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("glide", [False, True], ids=["hold", "glide"])
@pytest.mark.parametrize("key", list(CASES))
def test_passes_give_the_same_bits(tab, key, glide):
    """h1 and h2 are carried from pass to pass beside the phases, and a pass takes B from its own samples' rows"""
    case = CASES[key]
    whole = loop_of(tab, key, case, "70x101", glide)
    for per_pass in (1, 1000, 4097):
        got = render(tab, case, "70x101", glide, samples_per_pass=per_pass, form="loop" if per_pass == 1 else "relax")
        assert np.array_equal(bits(got), bits(whole)), per_pass


def test_output_shorter_and_longer_than_the_rendering(tab):
    case = CASES["chain3_gene_beside_fixed"]
    whole = loop_of(tab, "chain3_gene_beside_fixed", case, "7x101", False)
    covered = len(whole)
    for length in (covered - 5, covered + 5, 3, 0):
        for per_pass in (0, 500):
            got = render(tab, case, "7x101", False, form="relax", out_samples=length, samples_per_pass=per_pass)
            assert got.shape == (length,)
            assert np.array_equal(bits(got[:covered]), bits(whole[:length]))
            assert not bits(got[covered:]).any(), "the tail behind the rendering is exactly +0"


# ---- the rules -----------------------------------------------------------------------------------------------------------------
def test_rules_are_clean_under_asan_and_ubsan(tmp_path):
    """render_graph_genes_check, the gene-column helper, the form rule and the pass cap (csrc/sots_rules.h, pure host code) in
    a stand-alone program"""
    exe = tmp_path / "render_graph_genes_rules_san"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-o", str(exe),
                           os.path.join(ROOT, "tests", "render_graph_genes_rules_san.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert out.stdout.strip().startswith("ok: ") and out.stdout.strip().endswith(" checks")


# ---- the library and the host layer ------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_point(hip):
    lib = hip.load()
    assert "sots_render_graph_genes" in hip.EXPORTS and hasattr(lib, "sots_render_graph_genes")
    assert hasattr(hip.HipES, "render_graph_genes")
    with open(os.path.join(ROOT, "include", "sots_hip.h")) as f:
        text = f.read()
    assert "int sots_render_graph_genes(" in text and "sots_render_graph_genes        " in text  # the declaration, the table's row


def test_the_call_without_a_handle_is_refused(hip):
    """the only refusal that needs no handle: everything else is judged against the context's voice, N and D"""
    lib = hip.load()
    v = np.zeros((7, 5), np.float32)
    out = np.zeros(6 * 101 + N, np.float32)
    args = hip.RenderGraphFeedbackArgs(C.sizeof(hip.RenderGraphFeedbackArgs), 101, 0, 0, 0, 0)
    assert lib.sots_render_graph_genes(None, v.ctypes.data_as(C.c_void_p), v.nbytes, 7, C.byref(args), out.ctypes.data_as(C.c_void_p), out.size) == -1
    assert lib.sots_render_graph_genes(None, None, 0, 0, None, None, 0) == -1
    assert not out.any()


def test_render_mode_names(tmp_path):
    exe = tmp_path / "render_mode_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-o", str(exe), os.path.join(HOST, "render_mode_test.cpp")])
    good = {'{"renderMode": "graphGenes"}': "given 1 renderMode 7", '{"renderMode": "graphGenesGlide"}': "given 1 renderMode 8",
            '{"renderMode": "graphFeedbackGlide"}': "given 1 renderMode 6", '{"renderMode": "overlapAdd"}': "given 1 renderMode 0"}
    bad = ['{"renderMode": "graphgenes"}', '{"renderMode": "genes"}', '{"renderMode": "graphGenesglide"}', '{"renderMode": 7}']
    out = subprocess.run([str(exe)] + list(good) + bad, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = dict(l[5:].split(" -> ", 1) for l in out.stdout.splitlines())
    for text, want in good.items():
        assert got[text] == want, text
    for text in bad:
        assert got[text].startswith("refused: ") and '"graphGenes" or "graphGenesGlide"' in got[text], (text, got[text])


GRAPH = {"synth": "graph", "voiceGraph": CHAIN3}
PMAX_G = PMAX3 + [2.0]


@pytest.mark.parametrize("mode", ["graphGenes", "graphGenesGlide"])
@pytest.mark.parametrize("genes", [True, False], ids=["genes", "no-genes"])
def test_sots_match_takes_the_gene_modes_as_far_as_the_device(tmp_path, mode, genes):
    keys = dict(GRAPH, renderMatch=True, renderMode=mode)
    if genes:
        keys.update(voiceFeedbackGenes=[0, 1, 0], voiceFeedback=[0.5, 0, 0])
    out, wav = run_match(tmp_path, "far", keys, dims=7 if genes else 6, pmax=PMAX_G if genes else PMAX3, env=NO_DEVICE)
    assert out.returncode != 0 and "no HIP device" in out.stderr, out.stderr
    assert "renderMode" not in out.stderr and "voiceFeedbackGenes" not in out.stderr and not wav.exists()


@pytest.mark.parametrize("synth", ["2op", None])
@pytest.mark.parametrize("mode", ["graphGenes", "graphGenesGlide"])
def test_sots_match_refuses_the_gene_modes_for_a_fixed_voice_before_any_device_work(tmp_path, mode, synth):
    keys = {"renderMatch": True, "renderMode": mode}
    if synth:
        keys["synth"] = synth
    out, wav = run_match(tmp_path, "bad", keys, dims=4, pmax=[3520.0, 8.0, 3520.0, 1.0], env=NO_DEVICE)
    assert out.returncode != 0
    assert '"graphGenes" and "graphGenesGlide" need type.HIP.synth "graph"' in out.stderr, out.stderr
    assert "no HIP device" not in out.stderr and not wav.exists()


def test_the_fixed_index_modes_still_refuse_gene_operators_and_name_the_new_mode(tmp_path):
    keys = dict(GRAPH, voiceFeedbackGenes=[0, 1, 0], renderMatch=True, renderMode="graphFeedbackGlide")
    out, wav = run_match(tmp_path, "fb", keys, dims=7, pmax=PMAX_G, env=NO_DEVICE)
    assert out.returncode != 0
    assert 'every row has its own feedback index, which type.HIP.renderMode "graphFeedbackGlide" cannot render' in out.stderr, out.stderr
    assert '"graphGenes"' in out.stderr and "no HIP device" not in out.stderr and not wav.exists()
