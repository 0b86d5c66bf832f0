"""The run record on the device: best-ever individual, per-generation history and stop rules (sots_track and friends).

The checker is a TWIN context that runs the same generations one at a time, untracked, and reads the population back
after each: every record must describe exactly the rows the twin saw, and tracking must leave the population alone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PMAX = {0: [3520.0, 8.0, 3520.0, 1.0],
        1: [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0]}
SEED = 0x5EED0001
INF = np.float32(np.inf)


def chunk_targets(chunks, n, salt=0):
    """a different target per chunk (the targets of tests/test_gpu_batch.py)"""
    t = np.arange(n) / 44100.0
    out = np.empty((chunks, n), np.float32)
    for c in range(chunks):
        rng = np.random.default_rng(1000 * salt + c)
        f = 110.0 * (1 + c % 13) + 7.0 * salt
        out[c] = (0.6 * np.sin(2 * np.pi * f * t) + 0.3 * np.sin(2 * np.pi * 2.7 * f * t)
                  + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def same_record(a, b):
    """two best_ever() results: (values, steps, fitness, generation)"""
    return same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[2], b[2]) and a[3] == b[3]


def make(pkg, kind, log2n, parents, offspring, wg=16, chunk=0, target=None):
    es = pkg.HipES(parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=wg)
    es.set_target_audio(chunk_targets(chunk + 1, 1 << log2n)[chunk] if target is None else target)
    es.init_population(chunk)
    return es


def twin_trajectory(pkg, shape, gens, chunk=0, target=None, wg=16):
    """per generation g = 1..gens: the population (values, steps, fitness) an untracked context holds after it"""
    es = make(pkg, *shape, wg=wg, chunk=chunk, target=target)
    out = []
    for _ in range(gens):
        es.execute_generations(1)
        out.append(es.read_population())
    es.close()
    return out


def expected_best_ever(traj):
    """first minimum of row 0's fitness (NaN never wins, a tie keeps the older): (index, generation) or None"""
    best, at = INF, None
    for g, (_, _, f) in enumerate(traj):
        if f[0] < best:
            best, at = f[0], g
    return at


def check_history(hist, traj, parents, d, generations):
    """hist: records for the listed generations (1-based) of the twin's trajectory"""
    assert list(hist["generation"]) == list(generations)
    for rec, g in zip(hist, generations):
        v, s, f = traj[g - 1]
        at = expected_best_ever(traj[:g])
        ever = INF if at is None else traj[at][2][0]
        assert same_bits(rec["best_fitness"], f[0]), g
        assert same_bits(rec["parent_worst_fitness"], f[parents - 1]), g
        assert same_bits(rec["best_ever_fitness"], ever), g
        mean_f = f[:parents].astype(np.float64).mean()
        mean_s = s[:parents].astype(np.float64).mean(axis=0)
        # a pairwise fp32 sum of n <= 16384 terms errs by about log2(n) 2^-24 ~ 8e-7 relative; 1e-5 leaves ten times that
        assert abs(float(rec["parent_mean_fitness"]) - mean_f) <= 1e-5 * abs(mean_f), (g, rec["parent_mean_fitness"], mean_f)
        got = rec["mean_step"][:d].astype(np.float64)
        assert np.all(np.abs(got - mean_s) <= 1e-5 * np.abs(mean_s)), (g, got, mean_s)
        assert np.all(rec["mean_step"][d:] == 0) and np.all(rec["reserved"] == 0)


def check_best_ever(es, traj):
    v, s, f, g = es.best_ever()
    at = expected_best_ever(traj)
    assert at is not None
    tv, ts, tf = traj[at]
    assert g == at + 1, (g, at + 1)
    assert same_bits(f, tf[0]) and same_bits(v, tv[0]) and same_bits(s, ts[0])


# (voice, log2 N, parents, offspring)
SMALL = (0, 10, 32, 32)          # P = 64
SHIPPED = (1, 11, 16, 16)        # the shipped workload: 3-op, N = 2048, P = 32
MID = (0, 10, 512, 512)          # P = 1024
LARGE = (0, 10, 16384, 49152)    # P = 65536: the selection places rows 0..16383, the tail is lazy


# ---- 1. the population is untouched -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,wg,gens,sort_mode,plan", [
    (SMALL, 16, 12, None, None),
    (MID, 16, 6, None, None),
    (SHIPPED, 16, 12, None, None),
    (LARGE, 32, 4, 0, 1),   # lazy tail, selection by tiles
    (LARGE, 32, 4, 0, 2),   # lazy tail, selection between splitters
    (LARGE, 32, 4, 1, None),  # SOTS_SORT_FULL
])
def test_population_untouched(pkg, shape, wg, gens, sort_mode, plan):
    pops = []
    for tracked in (False, True):
        es = make(pkg, *shape, wg=wg)
        if sort_mode is not None:
            es.set_sort_mode(sort_mode)
        if plan is not None:
            es.set_select_plan(plan)
        if tracked:
            es.track(history_every=1, capacity=8)
        es.execute_generations(gens)
        if tracked:  # the record is read BEFORE the population: it must not need the lazy tail
            hist, taken = es.history(with_taken=True)
            assert taken == gens and hist["generation"][-1] == gens
        pops.append(es.read_population())
        es.close()
    for name, a, b in zip(("values", "steps", "fitness"), *pops):
        assert same_bits(a, b), name


# ---- 2. the history is exact ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,wg,gens", [(SMALL, 16, 20), (SHIPPED, 16, 20), ((0, 10, 1024, 3072), 32, 6), (LARGE, 32, 3),
                                           ((1, 11, 96, 160), 32, 5)])
def test_history_exact(pkg, shape, wg, gens):
    traj = twin_trajectory(pkg, shape, gens, wg=wg)
    es = make(pkg, *shape, wg=wg)
    es.track(history_every=1, capacity=gens)
    es.execute_generations(gens)
    hist, taken = es.history(with_taken=True)
    assert taken == gens
    check_history(hist, traj, shape[2], pkg.capi.SYNTH_DIMS[shape[0]], range(1, gens + 1))
    check_best_ever(es, traj)
    es.close()


def test_history_every_and_ring(pkg):
    gens = 20
    traj = twin_trajectory(pkg, SMALL, gens)
    es = make(pkg, *SMALL)
    es.track(history_every=5, capacity=16)
    es.execute_generations(gens)
    hist, taken = es.history(with_taken=True)
    assert taken == 4
    check_history(hist, traj, SMALL[2], 4, [5, 10, 15, 20])
    # a ring of 8 over 20 generations keeps the last 8, oldest first
    es.init_population(0)
    es.track(history_every=1, capacity=8)
    es.execute_generations(7)
    es.execute_generations(13)
    hist, taken = es.history(with_taken=True)
    assert taken == 20
    check_history(hist, traj, SMALL[2], 4, range(13, 21))
    es.close()


# ---- 3. best-ever ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 1, 2, 3])
def test_best_ever_is_the_first_minimum(pkg, chunk):
    """3-op N = 2048 P = 32, recombination block 16, 60 generations in three calls of 20"""
    traj = twin_trajectory(pkg, SHIPPED, 60, chunk=chunk)
    row0 = np.array([f[0] for _, _, f in traj])
    # precondition: the strategy is not elitist HERE - without a generation in which the best fitness rises, best-ever
    # equals the last row 0 all along and the test proves nothing (on the CPU oracle it rose in 20-29 of 60)
    rises = int(np.sum(row0[1:] > row0[:-1]))
    print(f"chunk {chunk}: best fitness rose in {rises} of 60 generations; final {row0[-1]:.6g}, best ever {row0.min():.6g}")
    assert rises >= 1
    es = make(pkg, *SHIPPED, chunk=chunk)
    es.track()
    for call in range(3):
        es.execute_generations(20)
        check_best_ever(es, traj[:20 * (call + 1)])
    es.close()


# ---- 4. staged loop versus fused loop ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,wg,gens", [(SMALL, 16, 10), (SHIPPED, 16, 10), ((0, 10, 1024, 3072), 32, 4)])
def test_staged_and_fused_loops_record_the_same(pkg, shape, wg, gens):
    fused, staged = make(pkg, *shape, wg=wg), make(pkg, *shape, wg=wg)
    for es in (fused, staged):
        es.track(history_every=1, capacity=gens)
    fused.execute_generations(gens)
    for _ in range(gens):
        staged.execute_generation()
    a, b = fused.history(), staged.history()
    assert len(a) == gens and a.tobytes() == b.tobytes()
    assert same_record(fused.best_ever(), staged.best_ever())
    # the single stages do not record
    staged.recombine(); staged.mutate(); staged.synthesise(); staged.window(); staged.fft(); staged.fitness(); staged.sort(); staged.rotate()
    assert staged.history(with_taken=True)[1] == gens
    fused.close(); staged.close()


# ---- 5. batch ------------------------------------------------------------------------------------------------------------
def test_batch_chunks_record_what_single_contexts_record(pkg):
    kind, log2n, parents, offspring = SHIPPED
    chunks, first, gens = 5, 2, 24
    targets = chunk_targets(chunks, 1 << log2n, salt=4)
    b = pkg.HipBatch(8, parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=16)
    b.track(history_every=2, capacity=8)
    b.set_target_audio(targets)
    b.init_population(first)
    b.execute_generations(gens)
    bv, bs, bf, bg = b.best_ever()
    for c in range(chunks):
        es = make(pkg, *SHIPPED, chunk=first + c, target=targets[c])
        es.track(history_every=2, capacity=8)
        es.execute_generations(gens)
        h, taken = b.history(c, with_taken=True)
        eh, etaken = es.history(with_taken=True)
        assert taken == etaken == gens // 2 and len(h) == 8
        assert h.tobytes() == eh.tobytes(), f"chunk {c}: history differs (means included)"
        v, s, f, g = es.best_ever()
        assert same_bits(bv[c], v) and same_bits(bs[c], s) and same_bits(bf[c], f) and bg[c] == g, f"chunk {c}: best-ever differs"
        assert g >= 1 and np.isfinite(f)
        es.close()
    # a re-targeted (now ragged: 3 of 8) batch starts cleared
    b.set_target_audio(chunk_targets(3, 1 << log2n, salt=5))
    v, s, f, g = b.best_ever()
    assert v.shape == (3, 6) and np.all(np.isposinf(f)) and np.all(g == 0) and not v.any() and not s.any()
    assert all(b.history(c, with_taken=True)[1] == 0 and len(b.history(c)) == 0 for c in range(3))
    b.init_population(0)
    b.execute_generations(4)
    assert np.all(np.isfinite(b.best_ever()[2])) and [r["generation"] for r in b.history(2)] == [2, 4]
    b.init_population(0)
    assert np.all(np.isposinf(b.best_ever()[2])) and len(b.history(0)) == 0
    b.close()


# ---- 6. stop rules -------------------------------------------------------------------------------------------------------
def model_generations_run(row0, max_generations, target, stall, interval):
    """the rule of include/sots_hip.h on a twin's row-0 fitness per generation: looks at block boundaries only"""
    g = 0
    while g < max_generations:
        g = min(g + interval, max_generations)
        best, at = INF, 0
        for i in range(g):
            if row0[i] < best:
                best, at = row0[i], i + 1
        if target is not None and target >= 0 and best <= np.float32(target):
            return g
        if stall and max(0, g - at) >= stall:
            return g
    return max_generations


STOP_CASES = [
    # (max generations, target, stall, interval)
    (50, 0.0, 0, 16),      # an unreachable target runs to the maximum, which is not a multiple of the interval
    (48, 0.0, 0, 16),
    (60, 1.0e30, 0, 8),    # a huge target stops at the first boundary
    (60, None, 5, 4),      # stall
    (60, None, 3, 1),
    (60, None, 12, 7),
]


@pytest.mark.parametrize("max_g,target,stall,interval", STOP_CASES)
def test_execute_until(pkg, max_g, target, stall, interval):
    traj = twin_trajectory(pkg, SHIPPED, max_g, chunk=1)
    row0 = [f[0] for _, _, f in traj]
    want = model_generations_run(row0, max_g, target, stall, interval)
    es = make(pkg, *SHIPPED, chunk=1)
    es.track()
    run = es.execute_until(max_g, target=target, stall=stall, check_every=interval)
    print(f"max {max_g} target {target} stall {stall} every {interval}: ran {run}")
    assert run == want and es.generation == want
    if target == 0.0:
        assert run == max_g
    if target == 1.0e30:
        assert run == interval
    for name, a, b in zip(("values", "steps", "fitness"), es.read_population(), traj[run - 1]):
        assert same_bits(a, b), name
    check_best_ever(es, traj[:run])
    es.close()


def test_execute_until_errors(pkg):
    es = make(pkg, *SMALL)
    with pytest.raises(pkg.SotsError) as e:
        es.execute_until(10, stall=2)   # no tracking
    assert e.value.code == -5
    with pytest.raises(pkg.SotsError) as e:
        es.history()                    # never enabled
    assert e.value.code == -5
    with pytest.raises(pkg.SotsError) as e:
        es.best_ever()
    assert e.value.code == -5
    es.track()
    with pytest.raises(pkg.SotsError) as e:
        es.execute_until(10, stall=2, check_every=0)
    assert e.value.code == -1
    with pytest.raises(pkg.SotsError) as e:
        es.history()                    # best-ever only
    assert e.value.code == -5
    # a rule with both conditions off never holds
    assert es.execute_until(9, check_every=4) == 9
    # byte counts are checked
    import ctypes as C
    v = np.empty(3, np.float32)
    assert es.L.sots_read_best_ever(es._h, v.ctypes.data_as(C.c_void_p), v.nbytes, None, 0, None, None) == -4
    es.close()


def test_batch_stops_when_the_rule_holds_for_every_chunk(pkg):
    kind, log2n, parents, offspring = SHIPPED
    chunks, max_g = 4, 60
    targets = chunk_targets(chunks, 1 << log2n)
    rows = [[f[0] for _, _, f in twin_trajectory(pkg, SHIPPED, max_g, chunk=c, target=targets[c])] for c in range(chunks)]

    def batch_stop(stall, interval):
        for g in range(interval, max_g + 1, interval):
            if all(_stalled(r, g, stall) for r in rows):
                return g
        return max_g

    # the first of a few rules under which, on the twins' trajectories, the batch stops before the maximum
    stall, interval = next((s, i) for s, i in [(6, 4), (4, 2), (3, 1), (2, 1)] if batch_stop(s, i) < max_g)
    want = batch_stop(stall, interval)
    single = [model_generations_run(r, max_g, None, stall, interval) for r in rows]
    print(f"stall {stall} every {interval}: per-chunk stops {single}, batch stops at {want}")
    b = pkg.HipBatch(chunks, parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=16)
    with pytest.raises(pkg.SotsError):
        b.execute_until(max_g, stall=stall, check_every=interval)  # no target yet / no tracking
    b.set_target_audio(targets)
    b.init_population(0)
    with pytest.raises(pkg.SotsError) as e:
        b.execute_until(max_g, stall=stall, check_every=interval)
    assert e.value.code == -5
    b.track()
    b.init_population(0)
    run = b.execute_until(max_g, stall=stall, check_every=interval)
    assert run == want and run >= max(single)
    # afterwards every chunk is where a single context is after `run` generations
    for c in range(chunks):
        es = make(pkg, *SHIPPED, chunk=c, target=targets[c])
        es.execute_generations(run)
        for a, x in zip(es.read_population(), b.read_population(c)):
            assert same_bits(a, x)
        es.close()
    b.close()


def _stalled(row0, g, stall):
    best, at = INF, 0
    for i in range(g):
        if row0[i] < best:
            best, at = row0[i], i + 1
    return max(0, g - at) >= stall


# ---- 7. clears -------------------------------------------------------------------------------------------------------------
def test_clears(pkg):
    es = make(pkg, *SMALL)
    es.track(history_every=1, capacity=4)

    def cleared():
        v, s, f, g = es.best_ever()
        hist, taken = es.history(with_taken=True)
        return np.isposinf(f) and g == 0 and not v.any() and not s.any() and taken == 0 and len(hist) == 0

    assert cleared()
    es.execute_generations(3)
    assert not cleared() and es.history(with_taken=True)[1] == 3
    # write_population and the generation counter leave the records alone
    before = es.best_ever()
    v, s, f = es.read_population()
    es.write_population(v, s, f)
    es.generation = 3
    assert same_record(before, es.best_ever())
    assert es.history(with_taken=True)[1] == 3
    es.init_population(0)
    assert cleared()
    es.execute_generations(2)
    es.set_target_audio(chunk_targets(2, 1024)[1])
    assert cleared()
    es.init_population(0)
    es.execute_generations(2)
    es.track(False)
    with pytest.raises(pkg.SotsError):
        es.best_ever()
    es.execute_generations(2)  # untracked again
    es.track(history_every=1, capacity=4)
    assert cleared()
    es.execute_generations(1)
    assert es.history()["generation"].tolist() == [5]
    es.close()


# ---- 8. sots_match ---------------------------------------------------------------------------------------------------------
def _lines(stdout, prefixes):
    return [l for l in stdout.splitlines() if l.startswith(prefixes)]


RESULT = ("Audio chunk", "Best parameters", "Best fitness", " p", "Overall best", " Fitness", "Generations run")


def _run_match(tmp_path, tag, hip_keys, chunks_in_flight):
    import json
    import os
    import struct
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg_dir = os.path.join(root, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
    exe = os.path.join(pkg_dir, "sots_match")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    audio = chunk_targets(12, 2048, salt=5).reshape(-1)
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
    return out.stdout, audio.reshape(12, 2048)


def _csv_by_chunk(path):
    rows = {}
    lines = path.read_text().splitlines()
    assert lines[0] == "chunk,generation,best,best_ever,parent_mean,parent_worst,step_0,step_1,step_2,step_3,step_4,step_5"
    for l in lines[1:]:
        rows.setdefault(int(l.split(",")[0]), []).append(l)
    return rows


def test_sots_match_best_ever_stall_and_history(tmp_path):
    outs, csvs = {}, {}
    for c in (1, 8):
        keys = {"returnBestEver": True, "stallGenerations": 10, "stopCheckInterval": 5, "historyEvery": 1,
                "historyPath": str(tmp_path / f"history{c}.csv")}
        outs[c], _ = _run_match(tmp_path, f"c{c}", keys, c)
        csvs[c] = _csv_by_chunk(tmp_path / f"history{c}.csv")
    a, b = _lines(outs[1], RESULT), _lines(outs[8], RESULT)
    runs = [int(l.split(":")[1]) for l in a if l.startswith("Generations run")]
    print("generations run per chunk:", runs)
    assert len(runs) == 12 and all(0 < r <= 120 and r % 5 == 0 for r in runs)
    assert a == b
    assert (tmp_path / "out_c1.wav").read_bytes() == (tmp_path / "out_c8.wav").read_bytes()
    # chunk by chunk, a chunk's history ends where it stopped; in flight it goes on to its batch's last boundary:
    # equal where the chunks stopped together, else equal over the common prefix of generations
    assert sorted(csvs[1]) == sorted(csvs[8]) == list(range(12))
    for c in range(12):
        one, many = csvs[1][c], csvs[8][c]
        assert len(one) == runs[c] and len(many) >= len(one) and len(many) % 5 == 0
        assert many[:len(one)] == one, f"chunk {c}"
        assert [int(l.split(",")[1]) for l in many] == list(range(1, len(many) + 1))
    # chunks of one batch share its stopping boundary
    assert len({len(csvs[8][c]) for c in range(8)}) == 1 and len({len(csvs[8][c]) for c in range(8, 12)}) == 1
    assert len(csvs[8][0]) == max(runs[:8]) and len(csvs[8][8]) == max(runs[8:])


def test_sots_match_without_the_new_keys_reports_the_last_row(pkg, tmp_path):
    """no new key: no new line, and the per-chunk fitness is row 0 of the last generation, as before"""
    stdout, chunks = _run_match(tmp_path, "plain", {}, 8)
    assert "Generations run" not in stdout
    got = [l for l in stdout.splitlines() if l.startswith("Best fitness")]
    want = []
    for c in range(12):
        es = make(pkg, *SHIPPED, chunk=c, target=chunks[c])
        es.execute_generations(120)
        want.append("Best fitness: %g" % float(es.read_fitness()[0]))
        es.close()
    assert got == want
    # and with returnBestEver alone the fitness printed is the minimum over the generations
    stdout, _ = _run_match(tmp_path, "ever", {"returnBestEver": True}, 8)
    ever = [float(l.split(":")[1]) for l in stdout.splitlines() if l.startswith("Best fitness")]
    last = [float(l.split(":")[1]) for l in got]
    assert len(ever) == 12 and all(e <= l for e, l in zip(ever, last)) and any(e < l for e, l in zip(ever, last))
