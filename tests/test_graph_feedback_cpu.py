"""CPU-side checks of the graph voice's per-operator feedback (sots_set_voice_feedback): the NumPy model
(tests/_graph_feedback_model.py) with all indices zero against the model of the waveforms (tests/_graph_waveforms_model.py),
which the oracle pins through the all-sine model; its vectorised form against its scalar restatement on mixed indices and
codes, NaN phases and negative minima included; the constant K; the spectral property the feature is for; the rule under
ASan + UBSan in a stand-alone program (tests/graph_feedback_san.cpp; nothing is loaded into Python under a sanitizer); the
host's own synthesiser against the model bit for bit through a stand-alone program (tests/graph_feedback_host.cpp); the
symbols; and what sots_match refuses before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _graph_feedback_model import (GRAPHS, K, SAW, SINE, W, edge_rows, graph_synth_feedback, graph_synth_feedback_scalar, graph_synth_waves,
                                   overflow_ranges, ranges)
from _graph_voice_match import CHAIN3, NO_DEVICE, run_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sots_set_voice_feedback", "sots_get_voice_feedback", "sots_batch_set_voice_feedback", "sots_batch_get_voice_feedback"]
BETAS = [0.0, 0.25, 1.0, 2.0]


@pytest.fixture(scope="module")
def table(O):
    return O.wavetable()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """bit for bit, a NaN matching any NaN"""
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def rotated_beta(ops, r):
    return [BETAS[(j + r) % 4] for j in range(ops)]


def rotated_codes(ops, r):
    return [(j + r) % 8 for j in range(ops)]


# ---- the constant ----
def test_the_constant_is_the_fp32_nearest_w_over_two_pi():
    assert K.dtype == np.float32 and K == np.float32(32768 / (2 * np.pi))
    assert int(np.array(K).view(np.uint32)) == 0x45a2f983 and float(K) == 5215.18896484375
    rules = open(os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd", "csrc", "sots_rules.h")).read()
    header = open(os.path.join(ROOT, "include", "sots_hip.h")).read()
    assert "0x1.45f306p+12f" in rules and "0x1.45f306p+12f" in header
    assert float.fromhex("0x1.45f306p+12") == float(K)


# ---- all indices zero: the model of the waveforms ----
@pytest.mark.parametrize("mixed", [False, True], ids=["sine", "mixed"])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_all_zero_is_the_model_of_the_waveforms(table, name, mixed):
    g = GRAPHS[name]
    assert len(GRAPHS) == 13
    waves = rotated_codes(g[0], 3) if mixed else [SINE] * g[0]
    pmin, pmax = ranges(g[0])
    v = edge_rows(2 * g[0], 6, 71)
    want = graph_synth_waves(g, waves, v, pmin, pmax, 256, table)
    got = graph_synth_feedback(g, waves, [0.0] * g[0], v, pmin, pmax, 256, table)
    assert np.array_equal(bits(got), bits(want)), name


# ---- vectorised against scalar ----
@pytest.mark.parametrize("rotation", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["2op", "chain3", "fan3", "stacks5", "seven", "additive8", "dense8"])
def test_mixed_indices_and_codes_vectorised_equal_scalar(table, name, rotation):
    g = GRAPHS[name]
    beta, waves = rotated_beta(g[0], rotation), rotated_codes(g[0], 2 * rotation + 1)
    pmin, pmax = ranges(g[0])  # negative minima: phases below 0
    v = edge_rows(2 * g[0], 4, 81 + rotation)
    got = graph_synth_feedback(g, waves, beta, v, pmin, pmax, 256, table)
    for r in range(v.shape[0]):
        want = graph_synth_feedback_scalar(g, waves, beta, v[r], pmin, pmax, 256, table)
        assert np.array_equal(bits(got[r]), bits(want)), (name, rotation, r)
    assert not np.array_equal(bits(got), bits(graph_synth_waves(g, waves, v, pmin, pmax, 256, table))), "the feedback changes nothing"


@pytest.mark.parametrize("name", ["fan3", "dense8"])
def test_nan_phases_behind_an_infinite_level_vectorised_equal_scalar(table, name):
    """overflow_ranges: operator 0's level is +inf, what it modulates has NaN phases; a NaN offset phase reads index 0"""
    g = GRAPHS[name]
    beta, waves = rotated_beta(g[0], 1), rotated_codes(g[0], 5)
    pmin, pmax = overflow_ranges(g[0])
    v = edge_rows(2 * g[0], 12, 91)
    got = graph_synth_feedback(g, waves, beta, v, pmin, pmax, 256, table)
    for r in range(v.shape[0]):
        want = graph_synth_feedback_scalar(g, waves, beta, v[r], pmin, pmax, 256, table)
        assert same(got[r], want), (name, r)
    assert (v[:, 0] * v[:, 1] > 0.5).any()


# ---- what it is for ----
def spectrum_db(row):
    n = row.size
    window = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)
    mag = np.abs(np.fft.rfft(row.astype(np.float64) * window))
    return 20 * np.log10(np.maximum(mag, 1e-300))


def off_harmonic(db, step):
    """the bins further than 4 from every multiple of step"""
    k = np.arange(db.size)
    distance = np.minimum(k % step, step - k % step)
    return db[distance > 4]


def test_a_feedback_sine_has_harmonics_and_no_aliases_where_a_saw_has_them(table):
    """N = 2048, Hann, the additive pair with the second carrier's level 0, operator 0 at bin 20 (430.6640625 Hz).  The
    bounds are conditions set before any measurement (an fp32 simulation gave harmonic 2 at -8.4 dB and the strongest
    non-harmonic bin at -93.6 dB with the index at 1, and -34 dB for the saw)"""
    g = GRAPHS["additive"]
    pmin, pmax = [0.0] * 4, [430.6640625, 1.0, 430.6640625, 0.0]
    v = np.ones((1, 4), np.float32)
    fed = spectrum_db(graph_synth_feedback(g, [SINE, SINE], [1.0, 0.0], v, pmin, pmax, 2048, table)[0])
    h1, h2 = fed[20], fed[40]
    print("harmonic 2, 3, 4 (dB):", h2 - h1, fed[60] - h1, fed[80] - h1, "strongest non-harmonic bin:", off_harmonic(fed, 20).max() - h1)
    assert -11.0 < h2 - h1 < -6.0
    assert off_harmonic(fed, 20).max() - h1 < -60.0
    saw = spectrum_db(graph_synth_feedback(g, [SAW, SINE], [0.0, 0.0], v, pmin, pmax, 2048, table)[0])
    print("saw, strongest non-harmonic bin:", off_harmonic(saw, 20).max() - saw[20])
    assert off_harmonic(saw, 20).max() - saw[20] > -40.0


# ---- the rule, stand-alone, under the sanitizers ----
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_feedback_rules_are_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "graph_feedback_san"
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", *SAN, "-o", str(exe),
                           os.path.join(ROOT, "tests", "graph_feedback_san.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert "graph feedback: 33 checks, 0 failures" in out.stdout, out.stdout


# ---- the host's own synthesiser against the model ----
@pytest.fixture(scope="module")
def host_synth(tmp_path_factory):
    d = tmp_path_factory.mktemp("graphfeedback")
    exe = d / "graph_feedback_host"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", *SAN[:3], "-o", str(exe),
                           os.path.join(ROOT, "tests", "graph_feedback_host.cpp")])

    def run(graph, waves, beta, values, pmin, pmax, log2n):
        ops, mods, carriers = graph
        head = np.zeros(20, np.uint32)
        head[0:3] = (log2n, ops, carriers)
        head[3:3 + ops] = mods
        head[11:11 + ops] = waves
        head[19] = values.shape[0]
        index = np.zeros(8, np.float32)
        if beta is None:
            index[0] = np.nan
        else:
            index[:ops] = beta
        lo, hi = np.zeros(16, np.float32), np.zeros(16, np.float32)
        lo[:2 * ops], hi[:2 * ops] = pmin, pmax
        case, out = d / "case.bin", d / "audio.f32"
        case.write_bytes(head.tobytes() + index.tobytes() + lo.tobytes() + hi.tobytes() + np.ascontiguousarray(values, np.float32).tobytes())
        res = subprocess.run([str(exe), str(case), str(out)], capture_output=True, text=True, env=ENV, timeout=300)
        assert res.returncode == 0, res.stderr[-4000:]
        return np.fromfile(out, np.float32).reshape(values.shape[0], 1 << log2n)

    return run


@pytest.mark.parametrize("name,rotation", [("2op", 1), ("chain3", 2), ("fan3", 0), ("stacks5", 3), ("dense8", 1), ("additive8", 2)])
def test_the_host_synthesiser_equals_the_model(table, host_synth, name, rotation):
    g = GRAPHS[name]
    beta, waves = rotated_beta(g[0], rotation), rotated_codes(g[0], rotation + 4)
    pmin, pmax = ranges(g[0])
    v = edge_rows(2 * g[0], 6, 101)
    got = host_synth(g, waves, beta, v, pmin, pmax, 8)
    want = graph_synth_feedback(g, waves, beta, v, pmin, pmax, 256, table)
    assert np.array_equal(bits(got), bits(want)), (name, beta, waves)


def test_the_host_synthesiser_without_indices_or_with_zeros_is_the_waveforms(table, host_synth):
    g = GRAPHS["chain3"]
    pmin, pmax = ranges(3)
    v = edge_rows(6, 6, 102)
    want = graph_synth_waves(g, [7, 1, 5], v, pmin, pmax, 256, table)
    assert np.array_equal(bits(host_synth(g, [7, 1, 5], None, v, pmin, pmax, 8)), bits(want))
    assert np.array_equal(bits(host_synth(g, [7, 1, 5], [0.0, 0.0, 0.0], v, pmin, pmax, 8)), bits(want))


# ---- the C-ABI without a device ----
def test_new_symbols_are_exported_and_declared(hip, pkg):
    lib = hip.load()
    header = open(os.path.join(ROOT, "include", "sots_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NEW:
        assert n in hip.EXPORTS and hasattr(lib, n), n
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
    assert not any(n.startswith("sots_group") and "feedback" in n for n in hip.EXPORTS)  # islands refuse the voice
    assert "Feed-forward only: no feedback" not in header and "sots_set_voice_feedback, below" in header
    for cls in (pkg.HipES, pkg.HipBatch):
        assert callable(cls.set_voice_feedback) and callable(cls.voice_feedback)
    assert not hasattr(pkg.HipGroup, "set_voice_feedback")


def test_null_handles_are_refused(hip):
    lib = hip.load()
    index = (C.c_float * 8)()
    assert lib.sots_set_voice_feedback(None, index, 2) == -1
    assert lib.sots_last_error(None).decode() == "null context"
    assert lib.sots_get_voice_feedback(None, index) == -1
    assert lib.sots_last_error(None).decode() == "null context"
    assert lib.sots_batch_set_voice_feedback(None, None, 0) == -1
    assert lib.sots_batch_last_error(None).decode() == "null batch"
    assert lib.sots_batch_get_voice_feedback(None, index) == -1
    assert lib.sots_batch_last_error(None).decode() == "null batch"


# ---- sots_match: what parameters.json can get wrong about the key, refused before any device work ----
GRAPH = {"synth": "graph", "voiceGraph": CHAIN3}
JSON_REFUSALS = [
    ({"synth": "2op", "voiceFeedback": [0.5, 0]}, 4, "type.HIP.voiceFeedback needs type.HIP.synth \"graph\""),
    ({"voiceFeedback": [0.5, 0]}, 4, "type.HIP.voiceFeedback needs type.HIP.synth \"graph\""),
    (dict(GRAPH, voiceFeedback=[0.5, 0]), 6, "type.HIP.voiceFeedback needs one number per operator (2 numbers, 3 operators)"),
    (dict(GRAPH, voiceFeedback=[0.5] * 4), 6, "type.HIP.voiceFeedback needs one number per operator (4 numbers, 3 operators)"),
    (dict(GRAPH, voiceFeedback=0.5), 6, "type.HIP.voiceFeedback needs one number per operator (not a list, 3 operators)"),
    (dict(GRAPH, voiceFeedback=[0, "1", 0]), 6, "type.HIP.voiceFeedback: an entry that is no number"),
    (dict(GRAPH, voiceFeedback=[0, 2.5, 0]), 6, "type.HIP.voiceFeedback: 2.500000 is outside 0..2"),
    (dict(GRAPH, voiceFeedback=[0, 0, -0.25]), 6, "type.HIP.voiceFeedback: -0.250000 is outside 0..2"),
    (dict(GRAPH, voiceFeedback=[1e300, 0, 0]), 6, "type.HIP.voiceFeedback: 10000000000000000525"),  # (beyond fp32: decided on the double)
    (dict(GRAPH, voiceFeedback=[0, 2.0000001, 0]), 6, "type.HIP.voiceFeedback: 2.000000 is outside 0..2"),
]


@pytest.mark.parametrize("keys,dims,text", JSON_REFUSALS)
def test_sots_match_refuses_before_any_device_work(tmp_path, keys, dims, text):
    # no device is visible to this run: anything that reached the device first would fail with ITS text
    out, wav = run_match(tmp_path, "bad", keys, dims=dims, env=NO_DEVICE)
    assert out.returncode != 0
    assert text in out.stderr, out.stderr
    assert "no HIP device" not in out.stderr and not wav.exists()


def test_sots_match_takes_a_good_key_as_far_as_the_device(tmp_path):
    out, wav = run_match(tmp_path, "good", dict(GRAPH, voiceFeedback=[1.0, 0, 2]), dims=6, env=NO_DEVICE)
    assert out.returncode != 0 and "no HIP device" in out.stderr and "voiceFeedback" not in out.stderr
