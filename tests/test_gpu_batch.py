"""Chunks in flight (sots_batch / HipBatch) against the sequential single context: chunk c of a batch must hold, bit for
bit, the whole population (values, steps, fitness) a HipES reaches with set_target_audio(chunk c),
init_population(first + c) and the same generations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PMAX = {0: [3520.0, 8.0, 3520.0, 1.0],
        1: [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0],
        2: [3520.0, 8.0, 3520.0, 1.0] + [0.0] * 8,
        3: [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0]}
SEED = 0x5EED0001


def chunk_targets(chunks, n, salt=0):
    """a different target per chunk: a few partials with chunk-dependent frequencies, and some noise"""
    t = np.arange(n) / 44100.0
    out = np.empty((chunks, n), np.float32)
    for c in range(chunks):
        rng = np.random.default_rng(1000 * salt + c)
        f = 110.0 * (1 + c % 13) + 7.0 * salt
        out[c] = (0.6 * np.sin(2 * np.pi * f * t) + 0.3 * np.sin(2 * np.pi * 2.7 * f * t)
                  + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return out


def sequential(pkg, kind, log2n, parents, offspring, targets, first, gens, arith=0):
    es = pkg.HipES(parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=16)
    if arith:
        es.set_synth_arithmetic(arith)
    pops = []
    for c, a in enumerate(targets):
        es.set_target_audio(a)
        es.init_population(first + c)
        es.execute_generations(gens)
        pops.append(es.read_population())
    es.close()
    return pops


def batched(b, targets, first, gens):
    b.set_target_audio(targets)
    b.init_population(first)
    b.execute_generations(gens)
    return [b.read_population(c) for c in range(len(targets))]


def assert_same(seq, bat, what=""):
    assert len(seq) == len(bat)
    for c, (x, y) in enumerate(zip(seq, bat)):
        for name, u, v in zip(("values", "steps", "fitness"), x, y):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), f"{what} chunk {c}: {name} differ"


# (voice, log2 N, parents, offspring, chunks, generations, first chunk index)
CASES = [
    (0, 10, 32, 32, 5, 3, 7),        # 2-op N = 1024 P = 64
    (0, 10, 32, 32, 1, 25, 0),       # one chunk
    (1, 11, 16, 16, 64, 3, 0),       # the shipped workload: 3-op N = 2048 P = 32 (k_fft_x, small-population variant)
    (1, 11, 16, 16, 5, 25, 2),
    (2, 10, 64, 64, 5, 1, 1),        # triple N = 1024 P = 128
    (3, 12, 32, 32, 64, 3, 3),       # 4-op N = 4096 P = 64: 4096 rows, k_fft_x's full workgroups
    (0, 8, 32, 32, 5, 25, 0),        # N = 256
    (0, 14, 16, 16, 5, 3, 0),        # N = 16384 (k_fft_big)
    (0, 10, 512, 512, 5, 3, 0),      # P = 1024: 5120 rows take k_fft's twelve-wavefront workgroups
]


@pytest.mark.parametrize("kind,log2n,parents,offspring,chunks,gens,first", CASES)
def test_batch_equals_sequential_contexts(pkg, kind, log2n, parents, offspring, chunks, gens, first):
    targets = chunk_targets(chunks, 1 << log2n)
    seq = sequential(pkg, kind, log2n, parents, offspring, targets, first, gens)
    b = pkg.HipBatch(chunks, parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED,
                     workgroup_size=16)
    bat = batched(b, targets, first, gens)
    assert_same(seq, bat)
    # read_best is row 0 of every chunk
    v, f = b.read_best()
    for c, (pv, _, pf) in enumerate(bat):
        assert np.array_equal(v[c], pv[0]) and np.array_equal(f[c:c + 1], pf[:1])
    b.close()


def test_ragged_and_reused_batch(pkg):
    kind, log2n, parents, offspring = 1, 11, 16, 16
    b = pkg.HipBatch(8, parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED,
                     workgroup_size=16)
    t1 = chunk_targets(5, 1 << log2n, salt=1)  # ragged: 5 of 8
    assert_same(sequential(pkg, kind, log2n, parents, offspring, t1, 4, 5), batched(b, t1, 4, 5), "ragged")
    # the used batch, re-targeted (more chunks now) and re-initialised, equals a fresh one
    t2 = chunk_targets(8, 1 << log2n, salt=2)
    used = batched(b, t2, 11, 4)
    fresh_b = pkg.HipBatch(8, parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED,
                           workgroup_size=16)
    assert_same(batched(fresh_b, t2, 11, 4), used, "reused")
    assert_same(sequential(pkg, kind, log2n, parents, offspring, t2, 11, 4), used, "reused vs sequential")
    # a few chunks fewer again: read_best covers the active ones only
    b.set_target_audio(t1[:3])
    b.init_population(0)
    b.execute_generations(2)
    v, f = b.read_best()
    assert v.shape == (3, 6) and f.shape == (3,)
    b.close()
    fresh_b.close()


@pytest.mark.parametrize("kind,log2n", [(0, 10), (1, 11)])
def test_batch_device_kernel_arithmetic(pkg, kind, log2n):
    parents, offspring, chunks, gens = 16, 16, 5, 3
    targets = chunk_targets(chunks, 1 << log2n, salt=3)
    seq = sequential(pkg, kind, log2n, parents, offspring, targets, 0, gens, arith=1)
    b = pkg.HipBatch(chunks, parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED,
                     workgroup_size=16)
    b.set_synth_arithmetic(1)
    assert_same(seq, batched(b, targets, 0, gens), "device arithmetic")
    b.close()


def _match_lines(stdout):
    """the per-chunk and overall result lines of sots_match (timing lines left out)"""
    keep = []
    for line in stdout.splitlines():
        if line.startswith(("Audio chunk", "Best parameters", "Best fitness", " p", "Overall best", " Fitness")):
            keep.append(line)
    return keep


def test_sots_match_chunks_in_flight(tmp_path):
    """sots_match on a 12-chunk WAV: chunksInFlight 1 (chunk by chunk) and 8 (batches of 8 and 4) print the same
    per-chunk and overall results and write byte-identical renderings"""
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
    cfg["evolutionary"].update({"numParents": 16, "numOffspring": 16, "numDimensions": 6, "numGenerations": 50,
                                "paramMins": [0.0] * 6, "paramMaxs": PMAX[1]})
    cfg["type"]["HIP"].update({"synth": "3op_series", "workgroupSize": 16})
    cfg["type"].update({"input": "audio", "audio": str(wav)})
    outs = {}
    for c in (1, 8):
        cfg["type"]["HIP"]["chunksInFlight"] = c
        cfg["general"]["outputAudioPath"] = str(tmp_path / f"out{c}.wav")
        p = tmp_path / f"parameters{c}.json"
        p.write_text(json.dumps(cfg))
        out = subprocess.run([exe, "-j", str(p)], capture_output=True, text=True, timeout=300, cwd=tmp_path)
        assert out.returncode == 0, out.stderr
        assert "Chunks matched per second: " in out.stdout
        outs[c] = out.stdout
    a, b = _match_lines(outs[1]), _match_lines(outs[8])
    assert sum(l.startswith("Audio chunk") for l in a) == 12
    assert a == b
    assert (tmp_path / "out1.wav").read_bytes() == (tmp_path / "out8.wav").read_bytes()


def test_batch_state_errors(pkg):
    b = pkg.HipBatch(4, 16, 16, synth_kind=0, audio_log2=10, param_max=PMAX[0], seed=SEED, workgroup_size=16)
    with pytest.raises(pkg.SotsError):
        b.init_population(0)  # no target yet
    with pytest.raises(pkg.SotsError):
        b.set_target_audio(chunk_targets(5, 1024))  # more chunks than max_chunks
    b.set_target_audio(chunk_targets(2, 1024))
    with pytest.raises(pkg.SotsError):
        b.read_population(2)  # only two active chunks
    with pytest.raises(pkg.SotsError):
        pkg.HipBatch(4, 16, 16, synth_kind=3, audio_log2=10, param_max=PMAX[3]).set_synth_arithmetic(1)
    b.close()
