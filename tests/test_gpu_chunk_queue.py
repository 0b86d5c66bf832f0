"""The chunk queue on the device (sots_batch_queue_*): M chunks through the S slots of a batch, a slot refilled as soon as its
chunk's stop rule holds.

The reference in every comparison is the SEQUENTIAL tracked context - sots_set_target, sots_init_population(first + k),
sots_execute_until - never the queue itself: chunk k's result must be what that context reports, bit for bit, whichever
slot the chunk ran in and whenever it started.  Targets are those of tools/track_overhead.py."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from track_overhead import targets  # noqa: E402

PMAX = {0: [3520.0, 8.0, 3520.0, 1.0],
        1: [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0]}
SEED = 0x5EED0001

# (voice, log2 N, parents, offspring, recombination block)
SHIPPED = (1, 11, 16, 16, 32)    # 3-op, N = 2048, P = 32: k_fft_x, whose per-(lane, register) target table the turnover rewrites
SMALL = (0, 10, 32, 32, 32)      # 2-op, N = 1024, P = 64: the N/2 bins
FULL = (0, 10, 512, 512, 32)     # 2-op, N = 1024, P = 1024: the largest chunk population
SHORT = (0, 8, 16, 16, 32)       # N = 256: k_fft_x with two points per lane
LONG = (0, 14, 16, 16, 32)       # N = 16384: k_fft_big

STALL = dict(target=None, stall=50, check_every=25)
NO_RULE = dict(target=None, stall=0, check_every=32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def make_batch(pkg, shape, slots, track=True):
    kind, log2n, parents, offspring, wg = shape
    b = pkg.HipBatch(slots, parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=wg)
    if track:
        b.track()
    return b


_REFERENCE = {}


def reference(pkg, shape, chunks, first, max_g, rule, arith=0):
    """chunk k = 0..chunks-1 on ONE sequential tracked context: (results as the queue's structured array, populations)"""
    key = (shape, first, max_g, tuple(sorted(rule.items())), arith)
    have = _REFERENCE.get(key)
    if have is not None and len(have[0]) >= chunks:
        return have[0][:chunks], have[1][:chunks]
    kind, log2n, parents, offspring, wg = shape
    d = pkg.capi.SYNTH_DIMS[kind]
    tg = targets(chunks, 1 << log2n)
    es = pkg.HipES(parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=wg)
    es.track()
    if arith:
        es.set_synth_arithmetic(arith)
    out = np.zeros(chunks, pkg.capi.CHUNK_RESULT_DTYPE)
    pops = []
    for k in range(chunks):
        es.set_target_audio(tg[k])
        es.init_population(first + k)
        # (a rule with both conditions off never holds: the context's form of rule = NULL)
        run = es.execute_until(max_g, target=rule["target"], stall=rule["stall"], check_every=rule["check_every"])
        v, s, f, g = es.best_ever()
        pop = es.read_population()
        r = out[k]
        r["generations_run"], r["best_ever_generation"], r["best_ever_fitness"], r["last_fitness"] = run, g, f, pop[2][0]
        r["best_ever_values"][:d], r["best_ever_steps"][:d], r["last_values"][:d] = v, s, pop[0][0]
        pops.append(pop)
    es.close()
    _REFERENCE[key] = (out, pops)
    return out, pops


def assert_same_results(got, want):
    assert len(got) == len(want)
    for k in range(len(want)):
        for name in ("generations_run", "best_ever_generation"):
            assert got[k][name] == want[k][name], (k, name, got[k][name], want[k][name])
        for name in ("best_ever_fitness", "last_fitness", "best_ever_values", "best_ever_steps", "last_values"):
            assert same_bits(got[k][name], want[k][name]), (k, name, got[k][name], want[k][name])


def run_queue(pkg, shape, slots, chunks, first, max_g, rule, arith=0, keep=None, batch=None):
    b = batch or make_batch(pkg, shape, slots)
    if arith:
        b.set_synth_arithmetic(arith)
    b.queue_targets_audio(targets(chunks, 1 << shape[1]))
    results, stats = b.queue_run(first, max_g, keep=keep, **rule)
    kept = b.queue_kept_population() if keep is not None else None
    if batch is None:
        b.close()
    return results, stats, kept


def check_against_reference(pkg, shape, slots, chunks, first, max_g, rule, arith=0):
    want, _ = reference(pkg, shape, chunks, first, max_g, rule, arith)
    got, stats, _ = run_queue(pkg, shape, slots, chunks, first, max_g, rule, arith)
    runs = want["generations_run"]
    print(f"shape {shape} S {slots} M {chunks} first {first} max {max_g} rule {rule}: generations_run {sorted(set(runs.tolist()))}, "
          f"global {stats['global_generations']}, chunk generations {stats['chunk_generations']}")
    assert_same_results(got, want)
    assert stats["slots"] == min(slots, chunks)
    assert stats["global_generations"] == pkg.HipBatch.queue_makespan(runs, slots)
    assert stats["chunk_generations"] == int(runs.astype(np.uint64).sum())
    return want, stats


# ---- 1. the turnover is really exercised, and exact, on the shipped shape ----------------------------------------------------
def test_stall_rule_on_the_shipped_shape_turns_slots_over(pkg):
    """64 chunks through 16 slots under a 50-generation stall rule looked at every 25 generations"""
    want, _ = reference(pkg, SHIPPED, 64, 0, 1000, STALL)
    runs = want["generations_run"].tolist()
    by_batch = sum(max(runs[i:i + 16]) for i in range(0, 64, 16))
    makespan = pkg.HipBatch.queue_makespan(runs, 16)
    print(f"reference generations_run: {runs}; batch by batch {by_batch}, queue {makespan}")
    # a condition on the REFERENCE's numbers: without a spread of stop generations no slot is ever refilled ahead of its batch
    assert len(set(runs)) >= 3
    assert makespan < by_batch
    check_against_reference(pkg, SHIPPED, 16, 64, 0, 1000, STALL)


# ---- 2. slots and chunks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots,chunks", [(s, m) for s in (1, 4, 16) for m in sorted({1, max(1, s - 1), s, 3 * s + 1})])
def test_slots_and_chunks(pkg, slots, chunks):
    check_against_reference(pkg, SHIPPED, slots, chunks, 0, 1000, STALL)


# ---- 3. shapes and rules ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,slots,chunks,max_g,rule,arith", [
    (SHIPPED, 4, 13, 200, dict(target=40.0, stall=0, check_every=25), 0),    # target only
    (SHIPPED, 4, 13, 200, dict(target=40.0, stall=50, check_every=25), 0),   # both
    (SHIPPED, 4, 13, 60, NO_RULE, 0),                                        # rule = NULL
    (SHIPPED, 4, 13, 110, STALL, 0),            # the maximum is no multiple of the interval: slots fall out of step
    (SHIPPED, 4, 13, 37, NO_RULE, 0),           # ... nor of the host's block without a rule
    (SHIPPED, 4, 13, 200, STALL, 1),            # SOTS_ARITH_DEVICE_KERNELS
    (SMALL, 4, 13, 300, STALL, 0),
    (SMALL, 4, 13, 200, dict(target=5.0, stall=40, check_every=10), 0),
    (FULL, 2, 5, 120, dict(target=None, stall=20, check_every=10), 0),
    (FULL, 2, 3, 24, NO_RULE, 0),
    (SHORT, 2, 5, 150, STALL, 0),
    (LONG, 2, 3, 100, dict(target=None, stall=20, check_every=10), 0),
])
def test_shapes_and_rules(pkg, shape, slots, chunks, max_g, rule, arith):
    check_against_reference(pkg, shape, slots, chunks, 0, max_g, rule, arith)


def test_first_chunk_index(pkg):
    check_against_reference(pkg, SMALL, 4, 9, 5, 300, STALL)
    # the initialisation really draws with first + k: chunk 0 of this run is not chunk 0 of a run that starts at 0
    a, _ = reference(pkg, SMALL, 1, 5, 300, STALL)
    b, _ = reference(pkg, SMALL, 1, 0, 300, STALL)
    assert not same_bits(a[0]["best_ever_values"], b[0]["best_ever_values"])


# ---- 4. the kept population ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["first", "middle", "last"])
def test_kept_population_is_the_reference_s_current_half_at_its_stop(pkg, which):
    slots, chunks = 4, 13
    keep = {"first": 0, "middle": chunks // 2, "last": chunks - 1}[which]
    want, pops = reference(pkg, SHIPPED, chunks, 0, 1000, STALL)
    got, _, kept = run_queue(pkg, SHIPPED, slots, chunks, 0, 1000, STALL, keep=keep)
    assert_same_results(got, want)
    for name, a, x in zip(("values", "steps", "fitness"), kept, pops[keep]):
        assert same_bits(a, x), (keep, name)


# ---- 5. reuse -------------------------------------------------------------------------------------------------------------------
def test_two_runs_on_one_handle_and_ordinary_calls_afterwards(pkg):
    slots, chunks = 4, 13
    want, _ = reference(pkg, SHIPPED, chunks, 0, 1000, STALL)
    b = make_batch(pkg, SHIPPED, slots)
    first, stats1, _ = run_queue(pkg, SHIPPED, slots, chunks, 0, 1000, STALL, batch=b)
    again, stats2 = b.queue_run(0, 1000, **STALL)  # the stored queue, run again
    assert first.tobytes() == again.tobytes() and stats1 == stats2
    assert_same_results(again, want)
    # after a run the batch has no active targets
    with pytest.raises(pkg.SotsError) as e:
        b.execute_generations(1)
    assert e.value.code == -5
    with pytest.raises(pkg.SotsError) as e:
        b.queue_kept_population()   # nothing was kept
    assert e.value.code == -5
    # ... and with targets again it computes what a fresh handle computes
    tg = targets(3, 2048)
    fresh = make_batch(pkg, SHIPPED, slots)
    for x in (b, fresh):
        x.set_target_audio(tg)
        x.init_population(2)
        x.execute_generations(30)
    for c in range(3):
        for a, y in zip(b.read_population(c), fresh.read_population(c)):
            assert same_bits(a, y), c
    for a, y in zip(b.best_ever(), fresh.best_ever()):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(y).view(np.uint32))
    # and a queue run after ordinary calls is the same again
    third, _ = b.queue_run(0, 1000, **STALL)
    assert third.tobytes() == first.tobytes()
    b.close(); fresh.close()


# ---- 6. state errors ------------------------------------------------------------------------------------------------------------
def test_state_errors(pkg):
    tg = targets(5, 2048)
    b = make_batch(pkg, SHIPPED, 4, track=False)
    with pytest.raises(pkg.SotsError) as e:
        b.queue_run(0, 100, **STALL)      # no tracking (and no queue)
    assert e.value.code == -5
    b.queue_targets_audio(tg)
    with pytest.raises(pkg.SotsError) as e:
        b.queue_run(0, 100, **STALL)      # no tracking
    assert e.value.code == -5 and "tracking" in str(e.value)
    b.track(history_every=1, capacity=8)
    with pytest.raises(pkg.SotsError) as e:
        b.queue_run(0, 100, **STALL)      # per-slot history rings are out of scope
    assert e.value.code == -5 and "history" in str(e.value)
    b.track()
    with pytest.raises(pkg.SotsError) as e:
        b.queue_run(0, 100, keep=5, **STALL)
    assert e.value.code == -1
    results, stats = b.queue_run(0, 100, **STALL)
    assert len(results) == 5 and stats["slots"] == 4
    with pytest.raises(pkg.SotsError) as e:
        b.queue_targets_spectra(np.zeros((2, 1000), np.float32))   # a wrong bin count
    assert e.value.code in (-1, -4)
    b.close()
    c = make_batch(pkg, SHIPPED, 4)
    with pytest.raises(pkg.SotsError) as e:
        c.queue_run(0, 100, **STALL)      # tracking, but nothing queued
    assert e.value.code == -5 and "queue" in str(e.value)
    c.close()


# ---- 7. sots_match ---------------------------------------------------------------------------------------------------------------
RESULT = ("Audio chunk", "Best parameters", "Best fitness", " p", "Overall best", " Fitness", "Generations run")


def _run_match(tmp_path, tag, hip_keys, chunks_in_flight):
    """the pattern of tests/test_gpu_run_record.py: 12 noisy chunks of N = 2048 from a float WAV file, 3-op voice, P = 32"""
    pkg_dir = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
    exe = os.path.join(pkg_dir, "sots_match")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    audio = targets(12, 2048).reshape(-1)
    audio = (audio / np.abs(audio).max() * 0.9).astype(np.float32)
    wav = tmp_path / "in.wav"
    with open(wav, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + audio.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3, 1, 44100, 44100 * 4, 4, 32))
        f.write(b"data" + struct.pack("<I", audio.nbytes) + audio.tobytes())
    cfg = json.load(open(os.path.join(pkg_dir, "parameters.json")))
    cfg["general"].update({"isDebug": True, "isBenchmarking": False})
    cfg["audio"]["audioLengthLog2"] = 11
    cfg["evolutionary"].update({"numParents": 16, "numOffspring": 16, "numDimensions": 6, "numGenerations": 120,
                                "paramMins": [0.0] * 6, "paramMaxs": PMAX[1]})
    cfg["type"]["HIP"].update({"synth": "3op_series", "workgroupSize": 16, "chunksInFlight": chunks_in_flight})
    cfg["type"]["HIP"].update(hip_keys)
    cfg["type"].update({"input": "audio", "audio": str(wav)})
    cfg["general"]["outputAudioPath"] = str(tmp_path / f"out_{tag}.wav")
    p = tmp_path / f"parameters_{tag}.json"
    p.write_text(json.dumps(cfg))
    out = subprocess.run([exe, "-j", str(p)], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert out.returncode == 0, out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith(RESULT)], (tmp_path / f"out_{tag}.wav").read_bytes()


def _per_chunk(lines):
    """the per-chunk result lines: everything in front of the closing "Overall best parameters found" section"""
    at = next(i for i, l in enumerate(lines) if l.startswith("Overall best"))
    return lines[:at], lines[at:]


@pytest.mark.parametrize("best_ever", [False, True])
@pytest.mark.parametrize("rule", ["stall", "none"])
def test_sots_match_prints_the_same_lines_through_the_queue(tmp_path, rule, best_ever):
    """The per-chunk result lines are the same on all three paths.  The closing section and the rendering come from the
    population the context is left with: the queue leaves the last chunk's population as it was when THAT CHUNK stopped,
    which is what the chunk-by-chunk loop leaves, so those two agree always.  The batch-by-batch path leaves it as it was
    when the chunk's BATCH stopped (Evolutionary_Strategy_HIP::matchChunksInFlight reads it after the batch's last block),
    so with a stop rule and the last row reported its closing section can differ from both; it is compared where it
    cannot: without a rule, or with the best-ever individual reported."""
    keys = {"returnBestEver": best_ever}
    if rule == "stall":
        keys.update({"stallGenerations": 10, "stopCheckInterval": 5})
    one, wav_one = _run_match(tmp_path, "one", keys, 1)                                 # chunk by chunk
    flight, wav_flight = _run_match(tmp_path, "flight", keys, 8)                        # chunks in flight, batch by batch
    queue, wav_queue = _run_match(tmp_path, "queue", dict(keys, chunkQueue=True), 8)    # ... through the queue
    runs = [int(l.split(":")[1]) for l in one if l.startswith("Generations run")]
    print(f"rule {rule} best-ever {best_ever}: generations run per chunk {runs}")
    assert len([l for l in one if l.startswith("Best fitness")]) == 12
    assert len(runs) == (12 if rule == "stall" else 0)
    (one_chunks, one_end), (flight_chunks, flight_end), (queue_chunks, queue_end) = _per_chunk(one), _per_chunk(flight), _per_chunk(queue)
    assert len(one_chunks) > 12 * 8 and len(one_end) == 8
    assert queue_chunks == flight_chunks == one_chunks
    assert queue_end == one_end and wav_queue == wav_one
    if rule == "none" or best_ever:
        assert flight_end == one_end and wav_flight == wav_one
