"""CPU-side checks of the graph voice's operator waveforms (sots_set_voice_waveforms): the derived tables
against the statements of the definition entry by entry; the NumPy model (tests/_graph_waveforms_model.py) against the
all-sine model the oracle pins (tests/_graph_voice_model.py) - with all codes sine on every graph, and with one code on all
operators against that model reading the derived table; its vectorised form against its scalar restatement on mixed codes;
the rule under ASan + UBSan in a stand-alone program (tests/graph_waveforms_san.cpp; nothing is loaded into Python under a
sanitizer); the host's own synthesiser against the model bit for bit through a stand-alone program
(tests/graph_waveforms_host.cpp); the symbols; and what sots_match refuses before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _graph_voice_match import CHAIN3, NO_DEVICE, run_match
from _graph_voice_model import graph_synth
from _graph_waveforms_model import (ABS, additive_synth_waves, ABS_EVEN, EVEN, GRAPHS, HALF, NAMES, PULSE, SAW, SINE, SQUARE, W, WAVES, edge_rows,
                                    graph_synth_waves, graph_synth_waves_scalar, ranges, shape_table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
NEW = ["sots_set_voice_waveforms", "sots_get_voice_waveforms", "sots_batch_set_voice_waveforms", "sots_batch_get_voice_waveforms"]


@pytest.fixture(scope="module")
def table(O):
    return O.wavetable()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the derived tables, entry by entry ----
def test_every_shape_is_the_statement_of_the_definition(table):
    t = np.asarray(table, np.float32)
    plus_zero, sign = np.uint32(0), np.uint32(0x80000000)
    tb = bits(t)
    shapes = {w: bits(shape_table(w, t)) for w in WAVES}
    saw = shape_table(SAW, t)
    for i in range(W):
        low = i < W // 2
        assert shapes[SINE][i] == tb[i]
        assert shapes[HALF][i] == (tb[i] if low else plus_zero)
        assert shapes[ABS][i] == tb[i] & ~sign
        assert shapes[PULSE][i] == (tb[i] & ~sign if (i & (W // 4)) == 0 else plus_zero)
        assert shapes[EVEN][i] == (tb[2 * i] if low else plus_zero)
        assert shapes[ABS_EVEN][i] == (tb[2 * i] & ~sign if low else plus_zero)
        assert shapes[SQUARE][i] == bits(np.float32(1.0 if low else -1.0))
        assert float(saw[i]) == i / 16384.0 - 1.0  # exact: i 2^-14 and the difference are fp32 numbers
    assert all(s.dtype == np.uint32 and s.shape == (W,) for s in shapes.values())
    # what "decided on the index" is for: the last entry of the sine table is tiny and of either sign, the shapes do not care
    assert abs(float(t[W - 1])) < 1e-6 and shapes[HALF][W - 1] == plus_zero and shapes[SQUARE][W - 1] == bits(np.float32(-1.0))
    assert shapes[PULSE][W // 4 - 1] == tb[W // 4 - 1] and shapes[PULSE][W // 4] == plus_zero and shapes[PULSE][W // 2] == tb[W // 2] & ~sign
    assert NAMES == ["sine", "half", "abs", "pulse", "even", "absEven", "square", "saw"]


# ---- the new model against the one the oracle pins ----
@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_all_sine_is_the_existing_model(table, name, negative):
    g = GRAPHS[name]
    assert len(GRAPHS) == 13
    pmin, pmax = ranges(g[0], negative=negative)
    v = edge_rows(2 * g[0], 6, 21)
    want = graph_synth(g, v, pmin, pmax, 256, table)
    got = graph_synth_waves(g, [SINE] * g[0], v, pmin, pmax, 256, table)
    assert np.array_equal(bits(got), bits(want)), name


@pytest.mark.parametrize("name", ["2op", "chain3", "two_mods", "stacks5", "dense8"])
@pytest.mark.parametrize("w", list(WAVES))
def test_one_code_on_all_operators_is_the_existing_model_on_the_derived_table(table, name, w):
    g = GRAPHS[name]
    pmin, pmax = ranges(g[0])
    v = edge_rows(2 * g[0], 6, 31 + w)
    want = graph_synth(g, v, pmin, pmax, 256, shape_table(w, table))
    got = graph_synth_waves(g, [w] * g[0], v, pmin, pmax, 256, table)
    assert np.array_equal(bits(got), bits(want)), (name, w)
    if w != SINE:
        assert not np.array_equal(bits(got), bits(graph_synth(g, v, pmin, pmax, 256, table))), (name, w)


@pytest.mark.parametrize("rotation", [0, 3, 5])
@pytest.mark.parametrize("name", ["2op", "chain3", "fan3", "stacks5", "seven", "additive8", "dense8"])
def test_mixed_codes_vectorised_equal_scalar(table, name, rotation):
    g = GRAPHS[name]
    waves = [(j + rotation) % 8 for j in range(g[0])]
    pmin, pmax = ranges(g[0])
    v = edge_rows(2 * g[0], 4, 41 + rotation)
    got = graph_synth_waves(g, waves, v, pmin, pmax, 256, table)
    for r in range(v.shape[0]):
        want = graph_synth_waves_scalar(g, waves, v[r], pmin, pmax, 256, table)
        assert np.array_equal(bits(got[r]), bits(want)), (name, rotation, r)


@pytest.mark.parametrize("name", ["additive", "additive8"])
def test_the_stacked_form_for_additive_graphs_is_the_model(table, name):
    """the GPU test's table walk at N = 32768 computes its reference with the operators as an array axis"""
    g = GRAPHS[name]
    waves = [(7 - j) % 8 for j in range(g[0])]
    v = edge_rows(2 * g[0], 5, 61)
    for pmin, pmax in (ranges(g[0]), ([0.0] * (2 * g[0]), [2 * 44100 / 32768, 1.0] * g[0])):
        want = graph_synth_waves(g, waves, v, pmin, pmax, 512, table)
        hit = np.zeros((g[0], W), bool)
        got = additive_synth_waves(waves, v, pmin, pmax, 512, table, hit)
        assert np.array_equal(bits(got), bits(want)), name
        assert hit[:, 0].all() and hit.sum() > g[0]


# ---- the rule, stand-alone, under the sanitizers ----
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_waveform_rules_are_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "graph_waveforms_san"
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", *SAN, "-o", str(exe),
                           os.path.join(ROOT, "tests", "graph_waveforms_san.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert "graph waveforms: 26 checks, 0 failures" in out.stdout


# ---- the host's own synthesiser against the model ----
@pytest.fixture(scope="module")
def host_synth(tmp_path_factory):
    d = tmp_path_factory.mktemp("graphwaves")
    exe = d / "graph_waveforms_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", *SAN[:3], "-o", str(exe),
                           os.path.join(ROOT, "tests", "graph_waveforms_host.cpp")])

    def run(graph, waves, values, pmin, pmax, log2n):
        ops, mods, carriers = graph
        head = np.zeros(20, np.uint32)
        head[0:3] = (log2n, ops, carriers)
        head[3:3 + ops] = mods
        head[11:19] = 0xFFFFFFFF if waves is None else list(waves) + [0] * (8 - ops)
        head[19] = values.shape[0]
        lo, hi = np.zeros(16, np.float32), np.zeros(16, np.float32)
        lo[:2 * ops], hi[:2 * ops] = pmin, pmax
        case, out = d / "case.bin", d / "audio.f32"
        case.write_bytes(head.tobytes() + lo.tobytes() + hi.tobytes() + np.ascontiguousarray(values, np.float32).tobytes())
        res = subprocess.run([str(exe), str(case), str(out)], capture_output=True, text=True, env=ENV, timeout=300)
        assert res.returncode == 0, res.stderr[-4000:]
        return np.fromfile(out, np.float32).reshape(values.shape[0], 1 << log2n)

    return run


@pytest.mark.parametrize("name,rotation", [("2op", 1), ("chain3", 6), ("fan3", 4), ("stacks5", 2), ("dense8", 0), ("additive8", 0)])
def test_the_host_synthesiser_equals_the_model(table, host_synth, name, rotation):
    g = GRAPHS[name]
    waves = [(j + rotation) % 8 for j in range(g[0])]
    pmin, pmax = ranges(g[0])
    v = edge_rows(2 * g[0], 6, 51)
    got = host_synth(g, waves, v, pmin, pmax, 8)
    want = graph_synth_waves(g, waves, v, pmin, pmax, 256, table)
    assert np.array_equal(bits(got), bits(want)), (name, waves)


def test_the_host_synthesiser_without_codes_is_all_sine(table, host_synth):
    g = GRAPHS["chain3"]
    pmin, pmax = ranges(3)
    v = edge_rows(6, 6, 52)
    want = graph_synth(g, v, pmin, pmax, 256, table)
    assert np.array_equal(bits(host_synth(g, None, v, pmin, pmax, 8)), bits(want))
    assert np.array_equal(bits(host_synth(g, [0, 0, 0], v, pmin, pmax, 8)), bits(want))


# ---- the C-ABI without a device ----
def test_new_symbols_are_exported_and_declared(hip, pkg):
    lib = hip.load()
    header = open(os.path.join(ROOT, "include", "sots_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NEW:
        assert n in hip.EXPORTS and hasattr(lib, n), n
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
    assert not any(n.startswith("sots_group") and "waveform" in n for n in hip.EXPORTS)  # islands refuse the voice
    assert [hip.WAVE_SINE, hip.WAVE_HALF, hip.WAVE_ABS, hip.WAVE_PULSE, hip.WAVE_EVEN, hip.WAVE_ABS_EVEN, hip.WAVE_SQUARE, hip.WAVE_SAW] == list(range(8))
    assert [hip.WAVE_NAMES[n] for n in NAMES] == list(range(8)) and len(hip.WAVE_NAMES) == 8
    for k, name in enumerate(["SINE", "HALF", "ABS", "PULSE", "EVEN", "ABS_EVEN", "SQUARE", "SAW"]):
        assert re.search(r"\bSOTS_WAVE_%s = %d\b" % (name, k), code), name
    for cls in (pkg.HipES, pkg.HipBatch):
        assert callable(cls.set_voice_waveforms) and callable(cls.voice_waveforms)
    assert not hasattr(pkg.HipGroup, "set_voice_waveforms")


def test_null_handles_are_refused(hip):
    lib = hip.load()
    codes = (C.c_uint32 * 8)()
    assert lib.sots_set_voice_waveforms(None, codes, 2) == -1
    assert lib.sots_last_error(None).decode() == "null context"
    assert lib.sots_get_voice_waveforms(None, codes) == -1
    assert lib.sots_last_error(None).decode() == "null context"
    assert lib.sots_batch_set_voice_waveforms(None, None, 0) == -1
    assert lib.sots_batch_last_error(None).decode() == "null batch"
    assert lib.sots_batch_get_voice_waveforms(None, codes) == -1
    assert lib.sots_batch_last_error(None).decode() == "null batch"


# ---- sots_match: what parameters.json can get wrong about the key, refused before any device work ----
GRAPH = {"synth": "graph", "voiceGraph": CHAIN3}
JSON_REFUSALS = [
    ({"synth": "2op", "voiceWaveforms": ["sine", "saw"]}, 4, "type.HIP.voiceWaveforms needs type.HIP.synth \"graph\""),
    ({"voiceWaveforms": ["sine", "saw"]}, 4, "type.HIP.voiceWaveforms needs type.HIP.synth \"graph\""),
    (dict(GRAPH, voiceWaveforms=["sine", "saw"]), 6, "type.HIP.voiceWaveforms needs one name per operator (2 names, 3 operators)"),
    (dict(GRAPH, voiceWaveforms=["sine"] * 4), 6, "type.HIP.voiceWaveforms needs one name per operator (4 names, 3 operators)"),
    (dict(GRAPH, voiceWaveforms="saw"), 6, "type.HIP.voiceWaveforms needs one name per operator (not a list, 3 operators)"),
    (dict(GRAPH, voiceWaveforms=["sine", "triangle", "saw"]), 6,
     "type.HIP.voiceWaveforms: \"triangle\" is no waveform (sine, half, abs, pulse, even, absEven, square, saw)"),
    (dict(GRAPH, voiceWaveforms=["sine", "Saw", "saw"]), 6, "type.HIP.voiceWaveforms: \"Saw\" is no waveform"),
    (dict(GRAPH, voiceWaveforms=["sine", 7, "saw"]), 6, "type.HIP.voiceWaveforms: an entry that is no string is no waveform"),
    # the graph's own shape check stays: the waveforms are a key beside voiceGraph, not a fourth key in it
    ({"synth": "graph", "voiceGraph": dict(CHAIN3, waveforms=["sine"] * 3)}, 6, "type.HIP.voiceGraph must be {\"operators\": n"),
]


@pytest.mark.parametrize("keys,dims,text", JSON_REFUSALS)
def test_sots_match_refuses_before_any_device_work(tmp_path, keys, dims, text):
    # no device is visible to this run: anything that reached the device first would fail with ITS text
    out, wav = run_match(tmp_path, "bad", keys, dims=dims, env=NO_DEVICE)
    assert out.returncode != 0
    assert text in out.stderr, out.stderr
    assert "no HIP device" not in out.stderr and not wav.exists()


def test_sots_match_takes_a_good_key_as_far_as_the_device(tmp_path):
    out, wav = run_match(tmp_path, "good", dict(GRAPH, voiceWaveforms=["saw", "half", "absEven"]), dims=6, env=NO_DEVICE)
    assert out.returncode != 0 and "no HIP device" in out.stderr and "voiceWaveforms" not in out.stderr
