"""CPU checks of the phase-continuous rendering of the operator-graph voice with feedback: the NumPy model's
two statements of the chain against each other, its anchors in the model without feedback, the pass sizes, the comb filter of
the overlap-add rendering that it removes, one row against the graph voice itself, what the GPU tests' rows cover, the argument
rules under sanitizers, the library's export and the renderMode names of the host layer.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _graph_feedback_model as FM  # noqa: E402
import _graph_waveforms_model as WM  # noqa: E402
import _render_graph_continuous_model as GM  # noqa: E402
import _render_graph_feedback_model as RM  # noqa: E402
import _render_model as M  # noqa: E402
from _graph_voice_match import CHAIN3, NO_DEVICE, run_match  # noqa: E402
from _render_graph_feedback_cases import BASE, BASE_SHAPE, CHAIN3_CARRY, SHARED, mixed_level_cases, waveform_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
HOST = os.path.join(PKG_DIR, "host")
GRAPHS = GM.GRAPHS
bits = RM.bits


@pytest.fixture(scope="module")
def tab(O):
    return O.wavetable()


def rows_of(ops, rows=7):
    return GM.graph_rows(ops, rows, 100 + ops)  # the GPU tests' rows


# ---- the two statements of the chain ----------------------------------------------------------------------------------------
LOOP_BETA = {"2op": [0.75, 1.0], "chain3": [0.5, 1.0, 2.0], "additive": [1.0, 0.5], "dense8": [0.5, 0, 0, 1.0, 0, 0, 0, 1.5]}
_LOOPS = {}


def loop_of(tab, name, glide):
    if (name, glide) not in _LOOPS:
        ops = GRAPHS[name][0]
        pmin, pmax = WM.ranges(ops)
        waves = GM.MIXED8 if name == "dense8" else None
        _LOOPS[(name, glide)] = RM.render(GRAPHS[name], waves, LOOP_BETA[name], rows_of(ops), pmin, pmax, tab, 256, 101, glide)
    return _LOOPS[(name, glide)]


@pytest.mark.parametrize("glide", [False, True])
@pytest.mark.parametrize("cap", [8, 4096])
@pytest.mark.parametrize("tile", [256, 1024])
@pytest.mark.parametrize("name", ["2op", "chain3", "additive", "dense8"])
def test_loop_and_relaxation_agree_bit_for_bit(tab, name, tile, cap, glide):
    ops = GRAPHS[name][0]
    pmin, pmax = WM.ranges(ops)
    waves = GM.MIXED8 if name == "dense8" else None
    sweeps = []
    got = RM.render(GRAPHS[name], waves, LOOP_BETA[name], rows_of(ops), pmin, pmax, tab, 256, 101, glide, form="relax", tile=tile, cap=cap,
                    sweeps=sweeps)
    want = loop_of(tab, name, glide)
    assert np.array_equal(bits(got), bits(want))
    assert np.abs(want).max() > 0.01
    flagged = sum(1 for b in LOOP_BETA[name] if b)
    assert len(sweeps) == flagged * -(-862 // tile) and all(1 <= s <= min(cap, tile) for _, s, _ in sweeps)


# ---- anchors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("glide", [False, True])
@pytest.mark.parametrize("name", ["chain3", "one_mod_two_carriers", "dense8"])
def test_without_feedback_it_is_the_model_of_4_16(tab, name, glide):
    ops = GRAPHS[name][0]
    pmin, pmax = WM.ranges(ops)
    waves = GM.MIXED8[:ops]
    want = GM.render(GRAPHS[name], waves, rows_of(ops), pmin, pmax, tab, 256, 101, glide)
    assert np.array_equal(bits(RM.render(GRAPHS[name], waves, None, rows_of(ops), pmin, pmax, tab, 256, 101, glide)), bits(want))
    # an index that is not 0, is accepted, goes through the chain - and whose offset always fixes to 0
    tiny = [1e-10] * ops
    assert np.float32(1e-10) != 0 and abs(float(np.float32(1e-10) * FM.K)) * 2.0 ** 17 < 0.5
    for form in ("loop", "relax"):
        signs = set()
        got = RM.render(GRAPHS[name], waves, tiny, rows_of(ops), pmin, pmax, tab, 256, 101, glide, form=form, signs=signs)
        assert np.array_equal(bits(got), bits(want)), form
        assert signs <= {0}


@pytest.mark.parametrize("glide", [False, True])
def test_passes_give_the_same_bits(tab, glide):
    """h1 and h2 are carried from pass to pass beside the phases"""
    name, n, hop = "chain3", 1024, 1000
    pmin, pmax = GM.audible_ranges(GRAPHS[name])
    values = GM.graph_rows(3, 7, 5)
    beta = [0.5, 0.0, 1.0]
    whole = RM.render(GRAPHS[name], [0, 3, 0], beta, values, pmin, pmax, tab, n, hop, glide)
    assert len(whole) == 6 * hop + n
    for per_pass in (1, 1000, 4097):
        got = RM.render(GRAPHS[name], [0, 3, 0], beta, values, pmin, pmax, tab, n, hop, glide, samples_per_pass=per_pass,
                        form="loop" if per_pass == 1 else "relax")
        assert np.array_equal(bits(got), bits(whole)), per_pass


# ---- the comb filter that it removes -----------------------------------------------------------------------------------------
def test_a_stationary_feedback_tone_is_not_comb_filtered(O, tab):
    """40 identical rows of the additive pair, both carriers at 473.7 Hz, level 1 and beta = 1, N = 2048, hop 512: successive
    rows are half a period apart and the overlap-add rendering cancels every odd harmonic - the fundamental with them - while
    the continuous rendering is the feedback voice itself.  Unlike the sine of 4.16 the comb does not leave silence: it
    passes the even harmonics, which a feedback operator has.  A feedback sine of index 1 has harmonic amplitudes
    2 J_n(n) / n = 0.880, 0.353, 0.206, 0.141, 0.105, 0.082 ... (n = 1, 2, ...), squares 0.774, 0.125, 0.042, 0.020, 0.011,
    0.007 ...: about 0.99 in all, so the voice's RMS is near sqrt(0.99 / 2) = 0.70, and the even ones carry 0.155 of it, so
    what a comb of half a period passes has sqrt(0.155 / 0.99) = 0.40 of the voice's RMS.  Asserted: an RMS within 0.05 of
    0.70 for the continuous rendering and below 0.45 of that for the overlap-add one, which nothing that keeps the
    fundamental (0.88 of the RMS) reaches.  Measured: interior RMS 0.266861 (overlap-add) against 0.677997 (continuous)."""
    n, hop = 2048, 512
    graph = GRAPHS["additive"]
    pmin, pmax = GM.audible_ranges(graph)
    row = np.array([[473.7 / 3520.0, 1.0, 473.7 / 3520.0, 1.0]] * 40, np.float32)
    beta = [1.0, 1.0]
    ola = M.overlap_add(FM.graph_synth_feedback(graph, [0, 0], beta, row, pmin, pmax, n, tab), hop, M.window32(O, n))
    cont = RM.render(graph, None, beta, row, pmin, pmax, tab, n, hop, form="relax")
    assert len(ola) == len(cont)
    a, b = GM.interior_rms(ola, n), GM.interior_rms(cont, n)
    print("interior RMS: overlap-add %.6f, continuous %.6f" % (a, b))
    assert abs(b - 0.70) < 0.05 and a < 0.45 * b


# ---- one row is the row's voice ------------------------------------------------------------------------------------------------
# As in 4.16: not graph_synth_feedback bit for bit (17 fractional phase bits against 8 near W), but close in the matcher's unit,
# the largest bin difference of the windowed magnitude spectra relative to the largest bin.  Measured between the two models on
# these rows (32 rows of 2op, N = 2048, genes in [0.05, 0.95), audible_ranges, feedback on the carrier): see the parameters;
# asserted: twice that, the project's margin.
ONE_ROW = [(0.5, 0.001774), (1.0, 0.002080)]  # (beta = 1 is not chaotic at this precision: both indices are asserted)


@pytest.mark.parametrize("beta,measured", ONE_ROW)
def test_one_row_is_the_feedback_voice_in_the_matchers_unit(O, tab, beta, measured):
    n, graph = 2048, GRAPHS["2op"]
    pmin, pmax = GM.audible_ranges(graph)
    rows = M.unit_rows(32, 4, 27)
    voice = FM.graph_synth_feedback(graph, [0, 0], [0.0, beta], rows, pmin, pmax, n, tab)
    worst = 0.0
    for v, a in zip(rows, voice):
        want = O.spectrum(a)
        got = O.spectrum(RM.render(graph, None, [0.0, beta], v[None, :], pmin, pmax, tab, n, n, form="relax"))
        worst = max(worst, float(np.abs(got - want).max() / want.max()))
    print("beta %g: largest relative bin difference %.6f" % (beta, worst))
    assert worst <= 2.0 * measured


# ---- what the GPU tests render (tests/test_gpu_render_graph_feedback.py) covers -----------------------------------------------
def render_case(tab, case, glide=False, **kw):
    name, waves, beta = case
    ops = GRAPHS[name][0]
    pmin, pmax = WM.ranges(ops)
    n, rows, hop = BASE_SHAPE
    return RM.render(GRAPHS[name], waves, beta, rows_of(ops, rows), pmin, pmax, tab, n, hop, glide, **kw)


def test_the_gpu_tests_rows_hit_the_cap_of_8_and_offsets_of_each_sign(tab):
    for case in BASE:
        sweeps, signs = [], set()
        render_case(tab, case, form="relax", tile=1024, cap=8, sweeps=sweeps)
        assert any(capped for _, _, capped in sweeps), case[0]
        render_case(tab, case, signs=signs)
        assert signs == {-1, 0, 1}, case[0]


def test_a_cap_of_4096_is_never_hit(tab):
    """the device's tiles hold 1024 samples, and after 1024 sweeps every sample of a tile is final"""
    name, waves, beta, rows, n, hop = CHAIN3_CARRY
    pmin, pmax = WM.ranges(3)
    sweeps = []
    RM.render(GRAPHS[name], waves, [0.5, 0.5, 0.5], rows_of(3, rows)[:20], pmin, pmax, tab, n, hop, form="relax", tile=1024, cap=4096, sweeps=sweeps)
    assert len(sweeps) == 3 * 5 and not any(capped for _, _, capped in sweeps)
    print("sweeps per tile at beta 0.5:", sorted(s for _, s, _ in sweeps))


@pytest.mark.parametrize("w", list(WM.WAVES))
def test_every_waveform_is_read_in_every_eighth_by_a_feedback_operator(tab, w):
    seen = {}
    render_case(tab, waveform_case(w), seen=seen)
    assert seen[w] == set(range(8))


def test_the_shared_kernel_cases_tell_feedback_from_none(tab):
    """what a stale t buffer, a stale h or a wrong source for a modulator's value would render differs from what is asserted"""
    name, n, hop, rows, per_pass = SHARED
    pmin, pmax = WM.ranges(3)
    plain = GM.render(GRAPHS[name], None, rows_of(3, rows), pmin, pmax, tab, n, hop)
    assert per_pass == 4096 < len(plain) < 2 * per_pass  # two passes, the first a whole tile of the scans
    for beta in ([0.0, 1.0, 0.0], [0.0, 0.0, 0.5]):
        fed = RM.render(GRAPHS[name], None, beta, rows_of(3, rows), pmin, pmax, tab, n, hop, samples_per_pass=per_pass)
        assert (RM.bits(fed) != RM.bits(plain)).mean() > 0.9
    for case in mixed_level_cases():
        name, waves, beta = case
        assert GRAPHS[name][1][3] & 0b111 == 0b111 and [b != 0 for b in beta[:3]] == [False, False, True]
        unfed = render_case(tab, (name, waves, None))
        assert (RM.bits(render_case(tab, case)) != RM.bits(unfed)).mean() > 0.4


# ---- the rules ---------------------------------------------------------------------------------------------------------------
def test_rules_are_clean_under_asan_and_ubsan(tmp_path):
    """render_graph_feedback_check, the pass cap and the form rule (csrc/sots_rules.h, pure host code) in a stand-alone program"""
    exe = tmp_path / "render_graph_feedback_rules_san"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-o", str(exe),
                           os.path.join(ROOT, "tests", "render_graph_feedback_rules_san.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert out.stdout.strip().startswith("ok: ") and out.stdout.strip().endswith(" checks")


# ---- the library and the host layer -----------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_point(hip):
    lib = hip.load()
    assert "sots_render_graph_feedback" in hip.EXPORTS and hasattr(lib, "sots_render_graph_feedback")
    assert hasattr(hip.HipES, "render_graph_feedback")
    with open(os.path.join(ROOT, "include", "sots_hip.h")) as f:
        text = f.read()
    assert "int sots_render_graph_feedback(" in text and "} sots_render_graph_feedback_args;" in text


def test_render_mode_names(tmp_path):
    exe = tmp_path / "render_mode_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-o", str(exe), os.path.join(HOST, "render_mode_test.cpp")])
    good = {'{"renderMode": "graphFeedback"}': "given 1 renderMode 5", '{"renderMode": "graphFeedbackGlide"}': "given 1 renderMode 6",
            '{"renderMode": "graphContinuousGlide"}': "given 1 renderMode 4", '{}': "given 0 renderMode 0"}
    bad = ['{"renderMode": "graphfeedback"}', '{"renderMode": "feedback"}', '{"renderMode": 5}']
    out = subprocess.run([str(exe)] + list(good) + bad, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = dict(l[5:].split(" -> ", 1) for l in out.stdout.splitlines())
    for text, want in good.items():
        assert got[text] == want, text
    for text in bad:
        assert got[text].startswith("refused: ") and '"graphFeedback" or "graphFeedbackGlide"' in got[text], (text, got[text])
        assert '"graphContinuous" or "graphContinuousGlide"' in got[text]


@pytest.mark.parametrize("synth,dims,pmax", [("2op", 4, [3520.0, 8.0, 3520.0, 1.0]), (None, 4, [3520.0, 8.0, 3520.0, 1.0])])
@pytest.mark.parametrize("mode", ["graphFeedback", "graphFeedbackGlide"])
def test_sots_match_refuses_the_feedback_modes_for_a_fixed_voice_before_any_device_work(tmp_path, mode, synth, dims, pmax):
    # no device is visible to this run: anything that reached the device first would fail with ITS text
    keys = {"renderMatch": True, "renderMode": mode}
    if synth:
        keys["synth"] = synth
    out, wav = run_match(tmp_path, "bad", keys, dims=dims, pmax=pmax, env=NO_DEVICE)
    assert out.returncode != 0
    assert '"graphFeedback" and "graphFeedbackGlide" need type.HIP.synth "graph"' in out.stderr, out.stderr
    assert "no HIP device" not in out.stderr and not wav.exists()


def test_sots_match_with_a_feedback_mode_and_feedback_gets_as_far_as_the_device(tmp_path):
    keys = {"synth": "graph", "voiceGraph": CHAIN3, "voiceFeedback": [0.0, 0.5, 0.75], "renderMatch": True, "renderMode": "graphFeedback"}
    out, wav = run_match(tmp_path, "far", keys, env=NO_DEVICE)
    assert out.returncode != 0 and "renderMode" not in out.stderr, out.stderr


def test_the_old_graph_modes_still_refuse_feedback_and_name_the_new_mode(tmp_path):
    keys = {"synth": "graph", "voiceGraph": CHAIN3, "voiceFeedback": [0.0, 0.5, 0.0], "renderMatch": True, "renderMode": "graphContinuousGlide"}
    out, wav = run_match(tmp_path, "fb", keys, env=NO_DEVICE)
    assert out.returncode != 0
    assert '"overlapAdd" renders such a voice' in out.stderr and '"graphFeedback"' in out.stderr, out.stderr
    assert "no HIP device" not in out.stderr and not wav.exists()
