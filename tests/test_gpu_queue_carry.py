"""Carried rows in the chunk queue on the device (sots_batch_queue_set_carry): inside a segment of L chunks a
chunk starts, in the slot and the launch in which its predecessor is retired, from the predecessor's best-ever record (row
0) and rows 1..R-1 of its sorted half, beside the fresh rows R..P-1.

The reference in every comparison is the SEQUENTIAL tracked context running the sequence the header gives as the definition
(read the state chunk k-1 left, set the target, init_population(first + k), write rows 0..R-1 back, execute_until) - never
the queue itself: chunk k's result must be what that context reports, bit for bit, whichever slot its segment ran in and
whenever it started.  Targets are the gliding track of tests/_carry_model.py at hop N/4; the shapes are those of
tests/test_gpu_chunk_queue.py."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from _carry_model import gliding_targets, gliding_track, segment_sums

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
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
RESULT_FLOATS = ("best_ever_fitness", "last_fitness", "best_ever_values", "best_ever_steps", "last_values")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def track_of(shape, chunks):
    """(the flat gliding signal, its hop N/4): what the queue takes; chunk k of it is gliding_targets(...)[k]"""
    n = 1 << shape[1]
    return gliding_track(chunks, n, n // 4), n // 4


def make_batch(pkg, shape, slots):
    kind, log2n, parents, offspring, wg = shape
    b = pkg.HipBatch(slots, parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=wg)
    b.track()
    return b


_CONTEXTS, _REFERENCE = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for es in _CONTEXTS.values():
        es.close()
    _CONTEXTS.clear()
    _REFERENCE.clear()


def context(pkg, shape, arith):
    es = _CONTEXTS.get((shape, arith))
    if es is None:
        kind, log2n, parents, offspring, wg = shape
        es = pkg.HipES(parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=wg)
        es.track()
        if arith:
            es.set_synth_arithmetic(arith)
        _CONTEXTS[(shape, arith)] = es
    return es


def reference(pkg, shape, chunks, first, max_g, rule, survivors, rows, segment, arith=0, targets=None):
    """the header's sequence on ONE sequential tracked context: (results as the queue's structured array, the population
    each chunk stopped with - its current half before any carrying touched it).  Computed once per setting and shared."""
    key = (shape, chunks, first, max_g, tuple(sorted(rule.items())), survivors, rows if rows else 0, segment if rows else 0, arith,
           None if targets is None else "one")
    have = _REFERENCE.get(key)
    if have is not None:
        return have
    d = pkg.capi.SYNTH_DIMS[shape[0]]
    n = 1 << shape[1]
    tg = gliding_targets(chunks, n, n // 4) if targets is None else targets
    es = context(pkg, shape, arith)
    es.set_survivors(survivors)
    out = np.zeros(chunks, pkg.capi.CHUNK_RESULT_DTYPE)
    pops = []
    for k in range(chunks):
        successor = rows > 0 and k % segment != 0
        if successor:   # the state chunk k-1 left
            pv, ps, _ = es.read_population()
            bv, bs, _, _ = es.best_ever()
        es.set_target_audio(tg[k])
        es.init_population(first + k)
        if successor:
            v, s, _ = es.read_population()
            v[:rows], s[:rows] = pv[:rows], ps[:rows]
            v[0], s[0] = bv, bs
            es.write_population(v, s, None)
        # (a rule with both conditions off never holds: the context's form of rule = NULL)
        run = es.execute_until(max_g, target=rule["target"], stall=rule["stall"], check_every=rule["check_every"])
        v, s, f, g = es.best_ever()
        pop = es.read_population()
        r = out[k]
        r["generations_run"], r["best_ever_generation"], r["best_ever_fitness"], r["last_fitness"] = run, g, f, pop[2][0]
        r["best_ever_values"][:d], r["best_ever_steps"][:d], r["last_values"][:d] = v, s, pop[0][0]
        pops.append(pop)
    _REFERENCE[key] = (out, pops)
    return out, pops


def assert_same_results(got, want):
    assert len(got) == len(want)
    for k in range(len(want)):
        for name in ("generations_run", "best_ever_generation"):
            assert got[k][name] == want[k][name], (k, name, got[k][name], want[k][name])
        for name in RESULT_FLOATS:
            assert same_bits(got[k][name], want[k][name]), (k, name, got[k][name], want[k][name])


def run_queue(pkg, shape, slots, chunks, first, max_g, rule, survivors, rows, segment, arith=0, keep=None, batch=None):
    b = batch or make_batch(pkg, shape, slots)
    if arith:
        b.set_synth_arithmetic(arith)
    b.set_survivors(survivors)
    b.queue_set_carry(rows, segment)
    signal, hop = track_of(shape, chunks)
    b.queue_targets_audio(signal, hop=hop)
    assert b.queued == chunks
    results, stats = b.queue_run(first, max_g, keep=keep, **rule)
    kept = b.queue_kept_population() if keep is not None else None
    if batch is None:
        b.close()
    return results, stats, kept


def check_against_reference(pkg, shape, slots, chunks, max_g, rule, survivors, rows, segment, arith=0, first=0):
    want, _ = reference(pkg, shape, chunks, first, max_g, rule, survivors, rows, segment, arith)
    got, stats, _ = run_queue(pkg, shape, slots, chunks, first, max_g, rule, survivors, rows, segment, arith)
    runs = want["generations_run"]
    print(f"shape {shape} S {slots} M {chunks} L {segment} R {rows} K {survivors} max {max_g} rule {rule}: generations_run {runs.tolist()}, "
          f"global {stats['global_generations']}")
    assert_same_results(got, want)
    length = min(segment, chunks)
    segments = -(-chunks // length)
    assert stats["slots"] == min(slots, segments)
    assert stats["global_generations"] == pkg.HipBatch.queue_makespan(segment_sums(runs, length), slots)
    assert stats["chunk_generations"] == int(runs.astype(np.uint64).sum())
    return want, got, stats


# ---- 1. results are the reference's, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("max_g,rule", [(200, STALL), (110, STALL), (37, NO_RULE)], ids=["stall200", "stall110", "none37"])
@pytest.mark.parametrize("survivors", [0, 1, 4])
@pytest.mark.parametrize("rows", [1, 2, 16])
@pytest.mark.parametrize("segment", [3, 4, 13, 20])
def test_shipped_shape(pkg, segment, rows, survivors, max_g, rule):
    """13 chunks in 4 slots: segments of 3 (a ragged last one), of 4, one segment of all, and a length beyond the queue; one
    row, two, and every parent; 110 is no multiple of the rule's interval and 37 none of the host's block"""
    check_against_reference(pkg, SHIPPED, 4, 13, max_g, rule, survivors, rows, segment)


def test_carrying_changes_the_results_from_the_first_successor_on(pkg):
    """(so that the comparisons above compare something: the reference with rows carried is not the plain sequence)"""
    carried, _ = reference(pkg, SHIPPED, 13, 0, 200, STALL, 1, 1, 3)
    plain, _ = reference(pkg, SHIPPED, 13, 0, 200, STALL, 1, 0, 0)
    for k in range(13):
        same = all(same_bits(carried[k][n], plain[k][n]) for n in RESULT_FLOATS)
        assert same == (k % 3 == 0), k


@pytest.mark.parametrize("shape,slots,chunks,segment,rows,survivors,max_g,rule,arith", [
    (SMALL, 4, 13, 3, 3, 1, 200, STALL, 0),
    (FULL, 2, 5, 3, 3, 1, 60, dict(target=None, stall=20, check_every=10), 0),
    (FULL, 2, 5, 3, 512, 1, 60, dict(target=None, stall=20, check_every=10), 0),   # every parent row: the refill starts half-way
    (SHORT, 2, 5, 2, 2, 1, 150, STALL, 0),
    (LONG, 2, 3, 3, 1, 1, 60, dict(target=None, stall=20, check_every=10), 0),
    (SHIPPED, 4, 13, 3, 2, 1, 200, STALL, 1),                                      # SOTS_ARITH_DEVICE_KERNELS
])
def test_shapes(pkg, shape, slots, chunks, segment, rows, survivors, max_g, rule, arith):
    check_against_reference(pkg, shape, slots, chunks, max_g, rule, survivors, rows, segment, arith)


def test_first_chunk_index(pkg):
    """the fresh rows of a successor are init_population(first + k)'s"""
    check_against_reference(pkg, SMALL, 4, 9, 200, STALL, 1, 2, 3, first=5)


# ---- 2. segments of one chunk: nothing is carried, through the new path --------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 16])
def test_segments_of_one_chunk_equal_a_run_without_carrying(pkg, rows):
    b = make_batch(pkg, SHIPPED, 4)
    off, stats_off, _ = run_queue(pkg, SHIPPED, 4, 13, 0, 200, STALL, 1, 0, 0, batch=b)
    on, stats_on, _ = run_queue(pkg, SHIPPED, 4, 13, 0, 200, STALL, 1, rows, 1, batch=b)
    assert b.queue_carry() == (rows, 1)
    b.close()
    assert on.tobytes() == off.tobytes() and stats_on == stats_off
    assert_same_results(on, reference(pkg, SHIPPED, 13, 0, 200, STALL, 1, 0, 0)[0])


# ---- 3. a chunk's result does not depend on the slots ------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [1, 2, 5, 8])
def test_slots_do_not_change_the_results(pkg, slots):
    want, got, stats = check_against_reference(pkg, SHIPPED, slots, 13, 200, STALL, 1, 2, 3)
    assert stats["slots"] == min(slots, 5)
    assert stats["global_generations"] == pkg.HipBatch.queue_makespan(segment_sums(want["generations_run"], 3), slots)
    assert stats["chunk_generations"] == int(want["generations_run"].astype(np.uint64).sum())


# ---- 4. one target: a successor starts no worse than its predecessor ended ---------------------------------------------------------
def test_on_one_target_the_best_ever_fitness_never_rises_along_a_segment(pkg):
    """eight chunks with the same target, one survivor, one carried row, one segment in one slot: the carried row is a bit
    copy of the predecessor's best-ever individual, evaluated in the same slot and row against the same table, and survives
    every generation unless something better takes its place"""
    one = gliding_targets(1, 2048, 512)[0]
    b = make_batch(pkg, SHIPPED, 4)
    b.set_survivors(1)
    b.queue_set_carry(1, 8)
    b.queue_targets_audio(np.stack([one] * 8))
    got, stats = b.queue_run(0, 200, **STALL)
    b.close()
    fit = [float(r["best_ever_fitness"]) for r in got]
    print(f"best-ever fitness along the segment: {fit}")
    assert stats["slots"] == 1
    assert all(y <= x for x, y in zip(fit, fit[1:])), fit
    want, _ = reference(pkg, SHIPPED, 8, 0, 200, STALL, 1, 1, 8, targets=np.stack([one] * 8))
    assert_same_results(got, want)


# ---- 5. the kept population ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [4, 5, 12], ids=["mid-segment", "last-of-segment", "last-chunk"])
def test_kept_population_is_the_reference_s_current_half_before_any_carrying(pkg, keep):
    """segments of 3: chunk 4 has a successor that overwrites row 0 and draws rows 2.. in the launch that retires it"""
    want, pops = reference(pkg, SHIPPED, 13, 0, 200, STALL, 1, 2, 3)
    got, _, kept = run_queue(pkg, SHIPPED, 4, 13, 0, 200, STALL, 1, 2, 3, keep=keep)
    assert_same_results(got, want)
    for name, a, x in zip(("values", "steps", "fitness"), kept, pops[keep]):
        assert same_bits(a, x), (keep, name)


# ---- 6. one handle: a carry run, carrying off, the ordinary calls ---------------------------------------------------------------------
def test_one_handle_through_a_carry_run_a_plain_run_and_the_ordinary_calls(pkg):
    b = make_batch(pkg, SHIPPED, 4)
    carried, _, _ = run_queue(pkg, SHIPPED, 4, 13, 0, 200, STALL, 1, 2, 3, batch=b)
    assert_same_results(carried, reference(pkg, SHIPPED, 13, 0, 200, STALL, 1, 2, 3)[0])
    again, _ = b.queue_run(0, 200, **STALL)   # a run keeps the setting
    assert again.tobytes() == carried.tobytes() and b.queue_carry() == (2, 3)
    b.queue_set_carry(0, 0)
    plain, stats = b.queue_run(0, 200, **STALL)
    assert b.queue_carry() == (0, 0) and stats["slots"] == 4
    assert_same_results(plain, reference(pkg, SHIPPED, 13, 0, 200, STALL, 1, 0, 0)[0])
    fresh = make_batch(pkg, SHIPPED, 4)
    fresh.set_survivors(1)
    signal, hop = track_of(SHIPPED, 13)
    fresh.queue_targets_audio(signal, hop=hop)
    untouched, stats_fresh = fresh.queue_run(0, 200, **STALL)
    assert plain.tobytes() == untouched.tobytes() and stats == stats_fresh
    # the ordinary batch calls, as on a fresh handle (sots_batch_execute_* ignores the setting: set it again first)
    b.queue_set_carry(2, 3)
    tg = gliding_targets(3, 2048, 512)
    for x in (b, fresh):
        x.set_target_audio(tg)
        x.init_population(2)
        x.execute_generations(30)
    for c in range(3):
        for a, y in zip(b.read_population(c), fresh.read_population(c)):
            assert same_bits(a, y), c
    for a, y in zip(b.best_ever(), fresh.best_ever()):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(y).view(np.uint32))
    b.close(); fresh.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_setting_and_the_getter_round_trips(pkg):
    b = make_batch(pkg, SHIPPED, 4)
    assert b.queue_carry() == (0, 0)
    b.queue_set_carry(16, 7)
    assert b.queue_carry() == (16, 7)
    for rows, segment, text in ((17, 7, "at most numParents = 16"), (3, 0, "segment_chunks must be at least 1"), (2**32 - 1, 1, "numParents")):
        with pytest.raises(pkg.SotsError) as e:
            b.queue_set_carry(rows, segment)
        assert e.value.code == -1 and text in str(e.value)
        assert b.queue_carry() == (16, 7)
    b.queue_set_carry(1, 2**32 - 1)
    assert b.queue_carry() == (1, 2**32 - 1)
    b.queue_set_carry(0, 9)   # off: the length is ignored and reported as 0
    assert b.queue_carry() == (0, 0)
    b.set_survivors(2)        # other settings leave it alone
    b.queue_set_carry(4, 5)
    b.set_survivors(0)
    b.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, 1e-3)
    signal, hop = track_of(SHIPPED, 3)
    b.queue_targets_audio(signal, hop=hop)
    assert b.queue_carry() == (4, 5)
    b.close()


# ---- 8. sots_match -----------------------------------------------------------------------------------------------------------------
def test_sots_match_writes_the_track_of_the_carry_run(pkg, tmp_path):
    """chunkQueue, hopSize, survivors and carryRows in type.HIP: the matchPath rows are the %.9g of the best-ever genes a
    HipBatch carry run of the same configuration reports (segmentChunks absent: ceil(chunks / chunksInFlight))"""
    chunks, hop, slots, gens = 9, 512, 4, 100
    exe = os.path.join(PKG_DIR, "sots_match")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    audio = gliding_track(chunks, 2048, hop)
    audio = (audio / np.abs(audio).max() * 0.9).astype(np.float32)
    wav = tmp_path / "in.wav"
    with open(wav, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + audio.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3, 1, 44100, 44100 * 4, 4, 32))
        f.write(b"data" + struct.pack("<I", audio.nbytes) + audio.tobytes())
    csv = tmp_path / "track.csv"
    cfg = json.load(open(os.path.join(PKG_DIR, "parameters.json")))
    cfg["general"].update({"isDebug": True, "isBenchmarking": False, "outputAudioPath": str(tmp_path / "out.wav")})
    cfg["audio"]["audioLengthLog2"] = 11
    cfg["evolutionary"].update({"numParents": 16, "numOffspring": 16, "numDimensions": 6, "numGenerations": gens,
                                "paramMins": [0.0] * 6, "paramMaxs": PMAX[1]})
    cfg["type"]["HIP"].update({"synth": "3op_series", "workgroupSize": 32, "seed": SEED, "chunksInFlight": slots, "chunkQueue": True,
                               "hopSize": hop, "survivors": 1, "carryRows": 2, "returnBestEver": True, "stallGenerations": 20,
                               "stopCheckInterval": 10, "matchPath": str(csv)})
    cfg["type"].update({"input": "audio", "audio": str(wav)})
    p = tmp_path / "parameters.json"
    p.write_text(json.dumps(cfg))
    out = subprocess.run([exe, "-j", str(p)], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert out.returncode == 0, out.stderr
    segment = -(-chunks // slots)
    assert f"Carried rows: 2, in segments of {segment} chunks" in out.stdout

    b = make_batch(pkg, SHIPPED, slots)
    b.set_survivors(1)
    b.queue_set_carry(2, segment)
    b.queue_targets_audio(audio, hop=hop)
    assert b.queued == chunks
    want, _ = b.queue_run(0, gens, stall=20, check_every=10)
    b.close()
    lines = csv.read_text().splitlines()
    assert len(lines) - 1 == chunks
    for k, line in enumerate(lines[1:]):
        cells = line.split(",")
        assert int(cells[0]) == k and int(cells[1]) == k * hop and int(cells[2]) == want[k]["generations_run"], (k, line)
        assert cells[4:10] == ["%.9g" % x for x in want[k]["best_ever_values"][:6]], (k, line)
