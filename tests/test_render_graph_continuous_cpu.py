"""CPU checks of the phase-continuous rendering of the operator-graph voice: the NumPy model against its own
per-sample loop and across pass sizes, its two anchors in the fixed voices' model, what the GPU tests' rows cover, the comb
filter of the overlap-add rendering that it removes, one row against the graph voice itself, the argument rules and the level
scheme under sanitizers, the library's export and the renderMode names of the host layer.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _graph_waveforms_model as WM  # noqa: E402
import _render_continuous_model as CM  # noqa: E402
import _render_graph_continuous_model as GM  # noqa: E402
import _render_model as M  # noqa: E402
from _graph_voice_match import CHAIN3, NO_DEVICE, run_match  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
HOST = os.path.join(PKG_DIR, "host")
GRAPHS = GM.GRAPHS


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def tab(O):
    return O.wavetable()


# ---- the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("glide", [False, True])
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("name", ["chain3", "two_mods", "one_mod_two_carriers", "dense8"])
def test_loop_and_cumsum_forms_agree_bit_for_bit(tab, name, mixed, glide):
    graph = GRAPHS[name]
    ops = graph[0]
    waves = GM.MIXED8[:ops] if mixed else None
    values = GM.graph_rows(ops, 6, 3 + ops)
    pmin, pmax = WM.ranges(ops)
    n, hop, samples = 64, 59, 300
    a = GM.render(graph, waves, values, pmin, pmax, tab, n, hop, glide, out_samples=samples)
    b = GM.render_loop(graph, waves, values, pmin, pmax, tab, n, hop, glide, out_samples=samples)
    assert np.array_equal(bits(a), bits(b))
    assert np.abs(a).max() > 0.01


@pytest.mark.parametrize("glide", [False, True])
def test_passes_give_the_same_bits(tab, glide):
    graph, n, hop = GRAPHS["stacks5"], 1024, 1000
    values = GM.graph_rows(5, 7, 5)
    pmin, pmax = WM.ranges(5)
    whole = GM.render(graph, GM.MIXED8[:5], values, pmin, pmax, tab, n, hop, glide)
    assert len(whole) == 6 * hop + n
    for per_pass in (0, 1, 1000, 4097):
        got = GM.render(graph, GM.MIXED8[:5], values, pmin, pmax, tab, n, hop, glide, samples_per_pass=per_pass)
        assert np.array_equal(bits(got), bits(whole)), per_pass


def test_levels():
    assert GM.levels(GRAPHS["chain8"]) == list(range(8)) and GM.levels(GRAPHS["additive8"]) == [0] * 8
    assert GM.levels(GRAPHS["stacks5"]) == [0, 1, 2, 0, 1] and GM.levels(GRAPHS["dense8"]) == [0, 1, 2, 3, 4, 5, 6, 6]


# ---- the anchors: the two fixed voices that are graphs, bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("glide", [False, True])
@pytest.mark.parametrize("hop", [256, 64, 101, 1])
@pytest.mark.parametrize("name,kind", [("2op", 0), ("triple", 2)])
def test_anchor_graphs_are_the_fixed_voices(tab, name, kind, hop, glide):
    n = 256
    values = CM.track_rows(kind, 7, 100 * kind + 8)
    pmax4 = CM.PMAX[kind]
    pairs = GRAPHS[name][0] // 2
    want = CM.render(kind, values, [0.0] * 4, pmax4, tab, n, hop, glide)
    got = GM.render(GRAPHS[name], None, values, [0.0] * (4 * pairs), pmax4 * pairs, tab, n, hop, glide)  # the ranges of genes 0..3 per pair
    assert np.array_equal(bits(got), bits(want))
    assert np.abs(want).max() > 0.01


# ---- what the GPU tests render (tests/test_gpu_render_graph_continuous.py) covers ---------------------------------------------
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_the_gpu_tests_rows_cover_negative_and_wrapping_increments(tab, name):
    graph = GRAPHS[name]
    ops = graph[0]
    wide = []
    pmin, pmax = WM.ranges(ops)
    GM.render(graph, None, GM.graph_rows(ops, 7, 100 + ops), pmin, pmax, tab, 256, 101, wide=wide)
    assert min(int(w.min()) for _, w, _ in wide) < 0, "no negative increment"
    if any(graph[1]):  # (a sum of unmodulated carriers has increments of at most c 3520 Hz)
        assert max(int(np.abs(w).max()) for _, w, _ in wide) >= 1 << 31, "no increment of magnitude 2^31 or more before the reduction"


@pytest.mark.parametrize("name", ["two_mods", "chain8"])
def test_the_overflow_ranges_make_cur_non_finite_and_fix_zero(tab, name):
    graph = GRAPHS[name]
    ops = graph[0]
    wide = []
    pmin, pmax = WM.overflow_ranges(ops)
    out = GM.render(graph, None, GM.graph_rows(ops, 7, 100 + ops), pmin, pmax, tab, 256, 101, wide=wide)
    bad = [(j, w, cur) for j, w, cur in wide if not np.isfinite(cur).all()]
    # (operator 0's own increment c f is beyond fix's range too: its phase stays 0, and 0 x inf is NaN)
    assert bad, "no non-finite cur"
    for _, w, cur in bad:
        assert not w[~np.isfinite(cur)].any(), "fix of a non-finite cur must be 0"
    assert np.isfinite(out).all() and np.abs(out).max() > 0.01  # operator 0 is never heard


@pytest.mark.parametrize("w", list(WM.WAVES))
def test_every_branch_of_every_waveform_is_read_as_modulator_and_as_carrier(tab, w):
    """every code's branches are decided by the index's half (HALF, EVEN, ABS_EVEN, SQUARE) or quarter (PULSE): all eight
    eighths of the table are read in both roles"""
    seen = {}
    pmin, pmax = WM.ranges(3)
    GM.render(GRAPHS["chain3"], GM.chain3_waves(w), GM.graph_rows(3, 7, 103), pmin, pmax, tab, 256, 101, seen=seen)
    assert seen[(w, "modulator")] == set(range(8)) and seen[(w, "carrier")] == set(range(8))


def test_the_mixed_setting_has_every_code(tab):
    assert sorted(GM.MIXED8) == list(range(8))
    carriers = GRAPHS["dense8"][2]
    assert {GM.MIXED8[j] for j in range(8) if carriers >> j & 1} == {2, 5}  # table shapes in the mix, SQUARE and SAW among the modulators


# ---- the comb filter that it removes -----------------------------------------------------------------------------------------
def test_a_stationary_tone_is_not_comb_filtered(O, tab):
    """40 identical rows of the additive pair, both carriers at 473.7 Hz and level 1, N = 2048, hop 512: successive rows are
    half a period apart, the overlap-add rendering cancels to silence, the continuous one is the sine (RMS 1 / sqrt 2)"""
    n, hop = 2048, 512
    graph = GRAPHS["additive"]
    pmin, pmax = GM.audible_ranges(graph)
    row = np.array([[473.7 / 3520.0, 1.0, 473.7 / 3520.0, 1.0]] * 40, np.float32)
    ola = M.overlap_add(WM.graph_synth(graph, row, pmin, pmax, n, tab), hop, M.window32(O, n))
    cont = GM.render(graph, None, row, pmin, pmax, tab, n, hop)
    assert len(ola) == len(cont)
    print("interior RMS: overlap-add %.6f, continuous %.6f" % (GM.interior_rms(ola, n), GM.interior_rms(cont, n)))
    assert GM.interior_rms(ola, n) < 0.01
    assert abs(GM.interior_rms(cont, n) - 2.0 ** -0.5) < 0.001


# ---- one row is the row's voice ------------------------------------------------------------------------------------------------
# Not graph_synth_waves bit for bit: the phase has 17 fractional bits where fp32 has 8 near W.  It must stay close in the unit
# the matcher uses: the largest bin difference of the windowed magnitude spectra, relative to the largest bin.  Measured on
# these rows (32 rows, N = 2048, genes in [0.05, 0.95), audible_ranges): see the parameters; asserted: twice that, the margin of
# DESIGN.md 4.10, so that a change of definition shows and rounding noise does not.
ONE_ROW = [("two_mods", None, 17, 0.00909), ("chain3", None, 18, 0.0488), ("2op", [WM.ABS, WM.HALF], 19, 0.000286)]


@pytest.mark.parametrize("name,waves,seed,measured", ONE_ROW)
def test_one_row_is_the_graph_voice_in_the_matchers_unit(O, tab, name, waves, seed, measured):
    n, graph = 2048, GRAPHS[name]
    ops = graph[0]
    pmin, pmax = GM.audible_ranges(graph)
    rows = M.unit_rows(32, 2 * ops, seed)
    voice = WM.graph_synth_waves(graph, waves or [0] * ops, rows, pmin, pmax, n, tab)
    worst = 0.0
    for v, a in zip(rows, voice):
        want = O.spectrum(a)
        got = O.spectrum(GM.render(graph, waves, v[None, :], pmin, pmax, tab, n, n))
        worst = max(worst, float(np.abs(got - want).max() / want.max()))
    print("%s: largest relative bin difference %.6f" % (name, worst))
    assert worst <= 2.0 * measured


# ---- the rules and the level scheme ----------------------------------------------------------------------------------------------
def test_rules_and_levels_are_clean_under_asan_and_ubsan(tmp_path):
    """render_graph_continuous_check, graph_levels and the pass cap (csrc/sots_rules.h, pure host code) in a stand-alone program"""
    exe = tmp_path / "render_graph_continuous_rules_san"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-o", str(exe),
                           os.path.join(ROOT, "tests", "render_graph_continuous_rules_san.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert out.stdout.strip() == "ok: 154 checks"


def test_the_models_levels_are_the_librarys(tmp_path):
    # the level counts restated in the stand-alone program above are the NumPy model's
    with open(os.path.join(ROOT, "tests", "render_graph_continuous_rules_san.cpp")) as f:
        text = f.read()
    for name, graph in GRAPHS.items():
        ops, mods, carriers = graph
        line = next(l for l in text.splitlines() if l.strip().startswith('{"%s",' % name))
        assert line.rstrip().endswith(", 0x%X, %d}," % (carriers, max(GM.levels(graph)) + 1)), line
        masks = [int(x, 0) for x in line[line.index("{", 5) + 1:line.index("}")].split(",")]
        assert masks == list(mods) and int(line.split(",")[1]) == ops, line


# ---- the library and the host layer -----------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_point(hip):
    lib = hip.load()
    assert "sots_render_graph_continuous" in hip.EXPORTS and hasattr(lib, "sots_render_graph_continuous")
    assert hasattr(hip.HipES, "render_graph_continuous")
    with open(os.path.join(ROOT, "include", "sots_hip.h")) as f:
        assert "int sots_render_graph_continuous(" in f.read()


def test_render_mode_names(tmp_path):
    exe = tmp_path / "render_mode_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-o", str(exe), os.path.join(HOST, "render_mode_test.cpp")])
    good = {'{"renderMode": "graphContinuous"}': "given 1 renderMode 3", '{"renderMode": "graphContinuousGlide"}': "given 1 renderMode 4",
            '{"renderMode": "continuousGlide"}': "given 1 renderMode 2", '{}': "given 0 renderMode 0"}
    bad = ['{"renderMode": "graphcontinuous"}', '{"renderMode": "graphGlide"}', '{"renderMode": 3}']
    out = subprocess.run([str(exe)] + list(good) + bad, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = dict(l[5:].split(" -> ", 1) for l in out.stdout.splitlines())
    for text, want in good.items():
        assert got[text] == want, text
    for text in bad:
        assert got[text].startswith("refused: ") and '"graphContinuous" or "graphContinuousGlide"' in got[text], (text, got[text])


@pytest.mark.parametrize("synth,dims,pmax", [("2op", 4, [3520.0, 8.0, 3520.0, 1.0]), ("3op_series", 6, [3520.0, 8.0] * 3), (None, 4, [3520.0, 8.0, 3520.0, 1.0])])
@pytest.mark.parametrize("mode", ["graphContinuous", "graphContinuousGlide"])
def test_sots_match_refuses_the_graph_modes_for_another_voice_before_any_device_work(tmp_path, mode, synth, dims, pmax):
    # no device is visible to this run: anything that reached the device first would fail with ITS text
    keys = {"renderMatch": True, "renderMode": mode}
    if synth:
        keys["synth"] = synth
    out, wav = run_match(tmp_path, "bad", keys, dims=dims, pmax=pmax, env=NO_DEVICE)
    assert out.returncode != 0
    assert '"graphContinuous" and "graphContinuousGlide" need type.HIP.synth "graph"' in out.stderr, out.stderr
    assert "no HIP device" not in out.stderr and not wav.exists()


def test_sots_match_refuses_the_graph_modes_with_feedback_before_any_device_work(tmp_path):
    keys = {"synth": "graph", "voiceGraph": CHAIN3, "voiceFeedback": [0.0, 0.5, 0.0], "renderMatch": True, "renderMode": "graphContinuous"}
    out, wav = run_match(tmp_path, "fb", keys, env=NO_DEVICE)
    assert out.returncode != 0
    assert "type.HIP.voiceFeedback" in out.stderr and '"overlapAdd" renders such a voice' in out.stderr, out.stderr
    assert "no HIP device" not in out.stderr and not wav.exists()


def test_sots_match_with_a_graph_mode_and_a_graph_gets_as_far_as_the_device(tmp_path):
    keys = {"synth": "graph", "voiceGraph": CHAIN3, "renderMatch": True, "renderMode": "graphContinuousGlide"}
    out, wav = run_match(tmp_path, "far", keys, env=NO_DEVICE)
    assert out.returncode != 0 and "renderMode" not in out.stderr, out.stderr
