"""CPU-side checks of carried rows in the chunk queue (sots_batch_queue_set_carry, sots_batch_queue_get_carry):
the symbols are exported and declared, null handles are refused, the oracle-composed reference sequence that the GPU tests
restate on a tracked context (tests/_carry_model.py) is the plain chunk sequence where nothing is carried and does on the
gliding track what the feature is for, sots_match refuses the keys it must before any device work, and the host-only code
(the refusals, the segment arithmetic the turnover kernel compiles, the loop bound) is clean under ASan + UBSan
(tests/queue_carry_san.cpp); sanitizers never run on the GPU."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from _carry_model import STALL_RULE, carry_sequence, gliding_targets, segment_sums, track_figures
from _survivors_model import PMAX, SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
CSRC = os.path.join(PKG_DIR, "csrc")
NEW = ["sots_batch_queue_set_carry", "sots_batch_queue_get_carry"]
SHIPPED = dict(kind=1, log2n=11, parents=16, offspring=16, block=32)


def test_new_symbols_are_exported_and_declared(hip):
    lib = hip.load()
    header = open(os.path.join(ROOT, "include", "sots_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NEW:
        assert n in hip.EXPORTS and hasattr(lib, n), n
        assert re.search(r"\bint\s+%s\s*\(" % n, header), n
    assert hasattr(hip.HipBatch, "queue_set_carry") and hasattr(hip.HipBatch, "queue_carry")


def test_null_handles_are_refused(hip):
    lib = hip.load()
    r, l = C.c_uint32(7), C.c_uint32(9)
    assert lib.sots_batch_queue_set_carry(None, 1, 4) == -1
    assert "null batch" in lib.sots_batch_last_error(None).decode()
    assert lib.sots_batch_queue_set_carry(None, 0, 0) == -1
    assert lib.sots_batch_queue_get_carry(None, C.byref(r), C.byref(l)) == -1
    assert "null batch" in lib.sots_batch_last_error(None).decode()
    assert (r.value, l.value) == (7, 9)


# ---- the model --------------------------------------------------------------------------------------------------------------
def oracle_es(O):
    w = SHIPPED
    return O.OracleES(w["parents"], w["offspring"], synth_kind=w["kind"], audio_log2=w["log2n"], param_max=PMAX[w["kind"]],
                      seed=SEED, recomb_block=w["block"])


def same(a, b):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        for name in x:
            assert np.array_equal(np.asarray(x[name], np.float32).view(np.uint32), np.asarray(y[name], np.float32).view(np.uint32)), (k, name)


def test_model_without_carried_rows_is_the_plain_chunk_sequence(O):
    """R = 0 at any L, and L = 1 at any R, against a sequence written out here without any carrying"""
    tg = gliding_targets(5)
    rule = dict(target=None, stall=10, check_every=5)
    ref = oracle_es(O)
    from _carry_model import run_chunk
    plain = []
    for k in range(5):
        ref.set_target_audio(tg[k])
        ref.init_population(3 + k)
        plain.append(run_chunk(ref, 1, 40, rule))
    for rows, segment in ((0, 0), (0, 3), (1, 1), (16, 1)):
        same(carry_sequence(oracle_es(O), tg, 3, 1, rows, segment, 40, rule), plain)
    # ... and carrying does change the sequence, from the first successor on and not before
    carried = carry_sequence(oracle_es(O), tg, 3, 1, 1, 5, 40, rule)
    same(carried[:1], plain[:1])
    assert not np.array_equal(carried[1]["best_ever_values"], plain[1]["best_ever_values"])


@pytest.fixture(scope="module")
def gliding(O):
    """the 24-chunk gliding track at hop 512, one survivor, the 50/25 stall rule, at most 1000 generations a chunk: the
    model's results with nothing carried and with one row carried through one segment"""
    tg = gliding_targets(24)
    return {r: carry_sequence(oracle_es(O), tg, 0, 1, r, 24, 1000, STALL_RULE) for r in (0, 1)}


def test_one_carried_row_on_the_gliding_track_needs_fewer_generations_and_gives_a_smoother_track(gliding):
    """(measured with this model: 4150 generations against 2300, mean best-ever fitness 0.1222 against 0.1104, mean
    |difference| of neighbouring genes 0.1624 against 0.0173: DESIGN.md 4.11 has the table)"""
    (gen0, fit0, jump0), (gen1, fit1, jump1) = track_figures(gliding[0]), track_figures(gliding[1])
    print(f"R = 0: {gen0} generations, mean best-ever {fit0:.4f}, mean |dgene| {jump0:.4f}; "
          f"R = 1: {gen1} generations, mean best-ever {fit1:.4f}, mean |dgene| {jump1:.4f}")
    assert gen1 < gen0
    assert jump1 < 0.5 * jump0


def test_segment_sums():
    assert segment_sums([75, 100, 125, 175, 75, 300, 25], 3) == [300, 550, 25]
    assert segment_sums([75, 100, 125], 1) == [75, 100, 125]
    assert segment_sums([75, 100, 125], 20) == [300]
    assert segment_sums([], 4) == []
    assert segment_sums(np.array([2**32 - 1, 2**32 - 1], np.uint32), 2) == [2 * (2**32 - 1)]


# ---- sots_match: what it refuses before any device work -----------------------------------------------------------------------
def _match(tmp_path, hip_keys, parents=16):
    exe = os.path.join(PKG_DIR, "sots_match")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    cfg = json.load(open(os.path.join(PKG_DIR, "parameters.json")))
    cfg["general"].update({"isDebug": False, "isBenchmarking": False, "outputAudioPath": str(tmp_path / "out.wav")})
    cfg["audio"]["audioLengthLog2"] = 11
    cfg["evolutionary"].update({"numParents": parents, "numOffspring": 16, "numDimensions": 6, "numGenerations": 10,
                                "paramMins": [0.0] * 6, "paramMaxs": PMAX[1]})
    cfg["type"]["implementation"] = "HIP"
    cfg["type"]["HIP"].update({"synth": "3op_series", "workgroupSize": 16, "chunksInFlight": 4, "device": 0})
    cfg["type"]["HIP"].update(hip_keys)
    p = tmp_path / "parameters.json"
    p.write_text(json.dumps(cfg))
    return subprocess.run([exe, "-j", str(p)], capture_output=True, text=True, timeout=120, cwd=tmp_path)


@pytest.mark.parametrize("keys,text", [
    (dict(chunkQueue=True, carryRows=17), "carryRows 17 exceeds evolutionary.numParents 16"),
    (dict(carryRows=1), "carryRows needs type.HIP.chunkQueue"),
    (dict(chunkQueue=False, carryRows=1, segmentChunks=4), "carryRows needs type.HIP.chunkQueue"),
    (dict(chunkQueue=True, carryRows=1, historyEvery=5, historyPath="history.csv"), "cannot be combined with type.HIP.historyPath"),
    (dict(chunkQueue=True, carryRows=1, segmentChunks=0), "segmentChunks must be a whole number, 1 or more"),
    (dict(chunkQueue=True, carryRows=1.5), "carryRows must be a whole number"),
    (dict(chunkQueue=True, carryRows=-1), "carryRows must be a whole number"),
])
def test_sots_match_refuses_the_keys_before_any_device_work(tmp_path, keys, text):
    """(on a machine without a GPU a configuration that passes these checks fails later, at the device, with another text)"""
    out = _match(tmp_path, keys)
    assert out.returncode == 1
    assert text in out.stderr, out.stderr
    assert "parameters.json: type.HIP." in out.stderr
    assert not (tmp_path / "out.wav").exists() and not (tmp_path / "history.csv").exists()


# ---- sanitizers: host code only ---------------------------------------------------------------------------------------------
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_carry_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    """queue_carry_check, queue_plan and queue_loop_bound (csrc/sots_rules.h) and the turnover's segment arithmetic
    (csrc/sots_stop_rule.h) as the library builds them, in a stand-alone program"""
    exe = tmp_path / "queue_carry_san"
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", *SAN, "-o", str(exe),
                           os.path.join(ROOT, "tests", "queue_carry_san.cpp"), os.path.join(CSRC, "sots_queue_host.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert "300 random cases, 0 failures" in out.stdout
