"""CPU-side checks of the analysis on the device: the fp64 model the GPU tests compare with
(tests/_analysis_model.py) against the oracle's own target spectrum, the new symbols and their null-handle refusals, the
pure-host checks of csrc/sots_rules.h in a stand-alone program under ASan + UBSan (tests/analysis_rules_san.cpp; sanitizers
never run on the GPU, and never on Python), and what sots_match refuses before any device work."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import _analysis_model as A
from _carry_model import gliding_track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
NEW = ["sots_batch_set_analysis", "sots_batch_get_analysis", "sots_batch_analyse_audio_hop", "sots_batch_queue_score_audio_hop"]


# ---- the model ----
@pytest.mark.parametrize("log2n", [8, 10, 11, 15])
def test_model_window_is_the_oracles(O, log2n):
    n = 1 << log2n
    w, wf = A.window(n)
    ow, owf = O.window(n)
    assert np.array_equal(w, np.asarray(ow, np.float64)) and np.float32(wf) == np.float32(owf)


@pytest.mark.parametrize("log2n,hop", [(8, 101), (10, 256), (11, 512), (11, 1), (15, 32768)])
def test_model_equals_the_oracles_target_spectrum(O, log2n, hop):
    """within the 1e-6 that read_target is held to against the same oracle (tests/test_gpu_parity.py)"""
    n, frames = 1 << log2n, 3
    x = gliding_track(frames, n, hop)
    m = A.magnitudes(x, n, hop, frames)
    assert m.shape == (frames, n // 2) and m.dtype == np.float64
    for f in range(frames):
        np.testing.assert_allclose(m[f], O.spectrum(x[f * hop:f * hop + n]), rtol=1e-6, atol=1e-9)


def test_model_frames_and_score():
    x = np.arange(20, dtype=np.float32)
    fr = A.frames(x, 8, 3, 5)
    assert fr.shape == (5, 8) and np.array_equal(fr[4], x[12:20]) and A.frame_count(20, 8, 3) == 5 and A.frame_count(7, 8, 3) == 0
    with pytest.raises(AssertionError):
        A.frames(x, 8, 3, 6)
    m, t = np.array([[1.0, 2.0, 4.0]]), np.array([[1.0, 1.0, 2.0]])
    assert A.score(m, t)[0] == 5.0 and A.score(m, t, [1.0, 0.0, 0.5])[0] == 2.0 and A.score(t, t, None, 1e-3)[0] == 0.0
    want = np.log((2.0 + 1e-3) / (1.0 + 1e-3)) ** 2 + np.log((4.0 + 1e-3) / (2.0 + 1e-3)) ** 2
    assert abs(A.score(m, t, None, 1e-3)[0] - want) < 1e-12


# ---- the C-ABI without a device ----
def test_symbols_and_null_handles(hip):
    lib = hip.load()
    for name in NEW:
        assert name in hip.EXPORTS and hasattr(lib, name)
    for name in ("set_analysis", "get_analysis", "analyse_audio_hop", "queue_score_audio_hop"):
        assert hasattr(hip.HipBatch, name)
    assert (hip.ANALYSIS_HOST, hip.ANALYSIS_DEVICE) == (0, 1)
    x = np.zeros(256, np.float32)
    p, m = x.ctypes.data_as(C.c_void_p), C.c_uint32(7)
    assert lib.sots_batch_set_analysis(None, 1) == -1 and "null batch" in lib.sots_batch_last_error(None).decode()
    assert lib.sots_batch_get_analysis(None, C.byref(m)) == -1 and m.value == 7
    assert lib.sots_batch_analyse_audio_hop(None, p, 256, 256, 1, p, 128) == -1
    assert lib.sots_batch_queue_score_audio_hop(None, p, 256, 256, p, 1) == -1


def test_header_says_the_device_targets_are_not_the_hosts_bits():
    text = open(os.path.join(ROOT, "include", "sots_hip.h")).read()
    at = text.index("enum sots_analysis")
    assert "NOT THE HOST'S BITS" in text[at - 1500:at] and "fp32" in text[at - 1500:at]


# ---- sanitizers: host code only ----
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_analysis_rules_are_clean_under_asan_and_ubsan(tmp_path):
    """analysis_mode_check, analysis_samples and analysis_frames_check (csrc/sots_rules.h) as the library builds them, in a
    stand-alone program: codes, texts and the uint64 arithmetic at the 2^28-sample and 2^30-byte edges"""
    exe = tmp_path / "analysis_rules_san"
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", *SAN, "-o", str(exe),
                           os.path.join(ROOT, "tests", "analysis_rules_san.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert "checks, 0 failures" in out.stdout


# ---- sots_match: what it refuses before any device work ----
def _match(tmp_path, hip_keys, parents=16, offspring=16):
    exe = os.path.join(PKG_DIR, "sots_match")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    cfg = json.load(open(os.path.join(PKG_DIR, "parameters.json")))
    cfg["general"].update({"isDebug": False, "isBenchmarking": False, "outputAudioPath": str(tmp_path / "out.wav")})
    cfg["audio"]["audioLengthLog2"] = 8
    cfg["evolutionary"].update({"numParents": parents, "numOffspring": offspring, "numDimensions": 4, "numGenerations": 10,
                                "paramMins": [0.0] * 4, "paramMaxs": [3520.0, 8.0, 3520.0, 1.0]})
    cfg["type"]["implementation"] = "HIP"
    cfg["type"]["HIP"].update({"synth": "2op", "workgroupSize": 16, "chunksInFlight": 4, "chunkQueue": True, "renderMatch": True, "device": 0})
    cfg["type"]["HIP"].update(hip_keys)
    p = tmp_path / "parameters.json"
    p.write_text(json.dumps(cfg))
    return subprocess.run([exe, "-j", str(p)], capture_output=True, text=True, timeout=120, cwd=tmp_path)


@pytest.mark.parametrize("keys,population,text", [
    (dict(deviceAnalysis=True, chunksInFlight=1), 32, "deviceAnalysis needs the chunks in flight"),
    (dict(deviceAnalysis=True, chunksInFlight=1, chunkQueue=False), 32, "deviceAnalysis needs the chunks in flight"),
    (dict(deviceAnalysis=True, numDevices=2), 32, "deviceAnalysis needs the chunks in flight"),
    (dict(deviceAnalysis=True), 2048, "deviceAnalysis needs the chunks in flight"),
    (dict(matchReport="report.csv", renderMatch=False), 32, "matchReport needs type.HIP.renderMatch"),
    (dict(matchReport="report.csv", chunkQueue=False), 32, "matchReport needs the chunk queue"),
    (dict(matchReport="report.csv", chunksInFlight=1), 32, "matchReport needs the chunk queue"),
    (dict(matchReport="report.csv", historyEvery=5, historyPath="history.csv"), 32, "matchReport needs the chunk queue"),
    (dict(matchReport="report.csv"), 2048, "matchReport needs the chunk queue"),
])
def test_sots_match_refuses_the_keys_before_any_device_work(tmp_path, keys, population, text):
    """(on a machine without a GPU a configuration that passes these checks fails later, at the device, with another text)"""
    out = _match(tmp_path, keys, parents=population // 2, offspring=population // 2)
    assert out.returncode == 1
    assert text in out.stderr and "parameters.json: type.HIP." in out.stderr, out.stderr
    assert not (tmp_path / "out.wav").exists() and not (tmp_path / "report.csv").exists() and not (tmp_path / "history.csv").exists()


def test_the_host_class_refuses_on_its_own(tmp_path):
    """Evolutionary_Strategy_HIP constructed directly (no parameters.json in front of it) throws the same way, before it
    asks for a device: a stand-alone g++ program against the library"""
    src = tmp_path / "driver.cpp"
    src.write_text('''#include <cstdio>
#include "Evolutionary_Strategy_HIP.hpp"
static int attempt(Evolutionary_Strategy_HIP_Arguments a, const char *want)
{
    try {
        Evolutionary_Strategy_HIP es(a);
    } catch (const std::exception &e) {
        printf("%s\\n", e.what());
        return std::string(e.what()).find(want) != std::string::npos ? 0 : 1;
    }
    return 1;
}
int main()
{
    Evolutionary_Strategy_HIP_Arguments a;
    a.es_args.pop.numParents = a.es_args.pop.numOffspring = 16;
    a.es_args.pop.numDimensions = 4;
    a.es_args.pop.populationLength = 32;
    a.es_args.numGenerations = 10;
    a.es_args.paramMin = {0, 0, 0, 0};
    a.es_args.paramMax = {3520.0f, 8.0f, 3520.0f, 1.0f};
    a.es_args.audioLengthLog2 = 8;
    a.verbose = false;
    a.logDirectory = "''' + str(tmp_path) + '''";
    int bad = 0;
    Evolutionary_Strategy_HIP_Arguments b = a;
    b.deviceAnalysis = true, b.chunksInFlight = 1;
    bad += attempt(b, "deviceAnalysis needs the chunks in flight");
    b = a, b.deviceAnalysis = true, b.chunksInFlight = 4, b.numDevices = 2;
    bad += attempt(b, "deviceAnalysis needs the chunks in flight");
    b = a, b.matchReport = "r.csv", b.chunksInFlight = 4, b.chunkQueue = true;
    bad += attempt(b, "matchReport needs renderMatch and the chunk queue");
    b = a, b.matchReport = "r.csv", b.chunksInFlight = 4, b.renderMatch = true;
    bad += attempt(b, "matchReport needs renderMatch and the chunk queue");
    return bad;
}
''')
    host = os.path.join(PKG_DIR, "host")
    exe = tmp_path / "driver"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", host, "-o", str(exe), str(src), "-L", PKG_DIR, "-lsots_hip",
                           "-Wl,-rpath," + PKG_DIR])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("Evolutionary_Strategy_HIP: ") == 4 and "device (" not in out.stdout
