"""CPU-side checks of the chunk queue (sots_batch_queue_*, sots_queue_makespan): the symbols are exported, bad calls are
refused with the right code and a text that names the fault, the result structure has the header's layout, and
sots_queue_makespan - pure host code - agrees with a min-heap model that belongs to this test.  The host-only code is
also built and run under ASan + UBSan (tests/queue_makespan_san.cpp); sanitizers never run on the GPU."""
import ctypes as C
import heapq
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd", "csrc")
NEW = ["sots_batch_queue_targets_spectra", "sots_batch_queue_targets_audio", "sots_batch_queue_run", "sots_batch_queue_results",
       "sots_batch_queue_read_kept_population", "sots_queue_makespan"]
NO_CHUNK = 0xFFFFFFFF


def test_new_symbols_are_exported(hip):
    lib = hip.load()
    for n in NEW:
        assert n in hip.EXPORTS and hasattr(lib, n), n


def _error(lib):
    return lib.sots_batch_last_error(None).decode()


def _stats(hip):
    s = hip.QueueStats()
    s.struct_size = C.sizeof(hip.QueueStats)
    return s


def test_null_batch_is_refused(hip):
    lib = hip.load()
    rule = hip.make_stop_rule(stall=50, check_every=25)
    mags = np.zeros(1024, np.float32)
    n = C.c_uint32(7)
    calls = [
        lambda: lib.sots_batch_queue_targets_spectra(None, mags.ctypes.data_as(C.c_void_p), mags.size, 1),
        lambda: lib.sots_batch_queue_targets_audio(None, mags.ctypes.data_as(C.c_void_p), mags.size, 1),
        lambda: lib.sots_batch_queue_run(None, 0, 100, C.byref(rule), NO_CHUNK, C.byref(_stats(hip))),
        lambda: lib.sots_batch_queue_run(None, 0, 100, None, NO_CHUNK, None),
        lambda: lib.sots_batch_queue_results(None, None, 0, C.byref(n)),
        lambda: lib.sots_batch_queue_read_kept_population(None, None, 0, None, 0, None, 0),
    ]
    for call in calls:
        assert call() == -1
        assert "null batch" in _error(lib)


def test_invalid_arguments_are_refused_with_a_text_that_names_them(hip):
    """arguments that need no handle are looked at before the handle, so a machine without a GPU can check them"""
    lib = hip.load()
    good = hip.make_stop_rule(stall=50, check_every=25)
    # a wrong struct_size in the rule
    rule = hip.make_stop_rule(stall=50, check_every=25)
    rule.struct_size = 12
    assert lib.sots_batch_queue_run(None, 0, 100, C.byref(rule), NO_CHUNK, None) == -1
    assert "stop rule" in _error(lib) and "struct_size" in _error(lib)
    # check_interval 0
    rule = hip.make_stop_rule(stall=50, check_every=0)
    assert lib.sots_batch_queue_run(None, 0, 100, C.byref(rule), NO_CHUNK, None) == -1
    assert "check_interval" in _error(lib)
    # a wrong struct_size in the stats
    stats = _stats(hip)
    stats.struct_size = 8
    assert lib.sots_batch_queue_run(None, 0, 100, C.byref(good), NO_CHUNK, C.byref(stats)) == -1
    assert "sots_queue_stats.struct_size" in _error(lib)
    # no generations
    assert lib.sots_batch_queue_run(None, 0, 0, C.byref(good), NO_CHUNK, None) == -1
    assert "max_generations" in _error(lib)
    # num_chunks 0
    mags = np.zeros(1024, np.float32)
    for fn in (lib.sots_batch_queue_targets_spectra, lib.sots_batch_queue_targets_audio):
        assert fn(None, mags.ctypes.data_as(C.c_void_p), mags.size, 0) == -1
        assert "num_chunks" in _error(lib)


def test_result_layouts(hip):
    assert C.sizeof(hip.ChunkResult) == 208
    assert hip.CHUNK_RESULT_DTYPE.itemsize == 208
    for name, offset in (("generations_run", 0), ("best_ever_generation", 4), ("best_ever_fitness", 8), ("last_fitness", 12),
                         ("best_ever_values", 16), ("best_ever_steps", 80), ("last_values", 144)):
        assert getattr(hip.ChunkResult, name).offset == offset and hip.CHUNK_RESULT_DTYPE.fields[name][1] == offset, name
    assert C.sizeof(hip.QueueStats) == 24 and hip.QueueStats.global_generations.offset == 8


# ---- sots_queue_makespan against a model ----------------------------------------------------------------------------------
def model_makespan(generations_run, slots):
    """a min-heap of the times at which the slots are free; chunks start in index order in the slot that is free first"""
    free_at = [0] * min(slots, max(1, len(generations_run)))
    heapq.heapify(free_at)
    last = 0
    for g in generations_run:
        end = heapq.heappop(free_at) + int(g)
        heapq.heappush(free_at, end)
        last = max(last, end)
    return last


def batch_by_batch(generations_run, slots):
    """today's schedule: batches of `slots` chunks, each running until its slowest chunk has stopped"""
    return sum(max(generations_run[i:i + slots]) for i in range(0, len(generations_run), slots))


def makespan(hip, generations_run, slots):
    g = np.ascontiguousarray(generations_run, np.uint32)
    out = C.c_uint64(123)
    rc = hip.load().sots_queue_makespan(g.ctypes.data_as(C.POINTER(C.c_uint32)), g.size, slots, C.byref(out))
    assert rc == 0
    return out.value


def test_makespan_agrees_with_the_model_on_random_cases(hip):
    rng = np.random.default_rng(0x5EED0001)
    for case in range(400):
        m = int(rng.integers(0, 300))
        slots = int(rng.integers(1, 70))
        interval = int(rng.choice([1, 7, 25, 32]))
        g = (rng.integers(0, 41, m) * interval).astype(np.uint32)
        if case % 5 == 0 and m:
            g[rng.integers(0, m)] = 2**32 - 1  # sums beyond 32 bits
        assert makespan(hip, g, slots) == model_makespan(g, slots), (case, m, slots)
        assert hip.HipBatch.queue_makespan(g, slots) == model_makespan(g, slots)


def test_makespan_hand_cases(hip):
    g = [75, 100, 125, 175, 75, 300, 25]
    assert makespan(hip, g, 1) == sum(g)                     # one slot: the sum
    assert makespan(hip, g, len(g)) == max(g)                # slots >= chunks: the max
    assert makespan(hip, g, 1000) == max(g)
    for m, s, count in ((16, 4, 100), (17, 4, 100), (1, 8, 33), (64, 16, 1000), (65, 16, 7)):
        assert makespan(hip, [count] * m, s) == -(-m // s) * count   # equal counts: ceil(M / S) x count
    assert makespan(hip, [], 3) == 0


# the CPU oracle on the shipped workload (3-op, N = 2048, 16 + 16 rows, recombination block 32, seed 0x5EED0001, the noisy
# chunks of tools/track_overhead.py): the first block boundary (interval 25, at most 1000 generations) at which a 50-generation
# stall rule holds for each of the first 16 chunks
ORACLE_STALL_50 = [75, 100, 75, 75, 125, 75, 75, 75, 75, 175, 75, 100, 75, 75, 75, 75]


def test_makespan_of_the_oracle_s_stall_50_stops(hip):
    assert sorted(set(ORACLE_STALL_50)) == [75, 100, 125, 175]
    assert batch_by_batch(ORACLE_STALL_50, 4) == 475
    assert makespan(hip, ORACLE_STALL_50, 4) == 375
    assert model_makespan(ORACLE_STALL_50, 4) == 375


def test_makespan_rejects_bad_arguments(hip):
    lib = hip.load()
    g = np.array([1, 2, 3], np.uint32)
    out = C.c_uint64(9)
    assert lib.sots_queue_makespan(g.ctypes.data_as(C.POINTER(C.c_uint32)), 3, 0, C.byref(out)) == -1 and out.value == 0
    assert lib.sots_queue_makespan(None, 3, 2, C.byref(out)) == -1
    assert lib.sots_queue_makespan(g.ctypes.data_as(C.POINTER(C.c_uint32)), 3, 2, None) == -1
    with pytest.raises(hip.SotsError):
        hip.HipBatch.queue_makespan(g, 0)


# ---- sanitizers: host code only ---------------------------------------------------------------------------------------------
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_queue_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    """csrc/sots_queue_host.cpp as the library builds it, and the stop-rule arithmetic the turnover kernel shares with the host"""
    exe = tmp_path / "queue_makespan_san"
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", *SAN, "-o", str(exe),
                           os.path.join(ROOT, "tests", "queue_makespan_san.cpp"), os.path.join(CSRC, "sots_queue_host.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert "300 random cases, 0 failures" in out.stdout
