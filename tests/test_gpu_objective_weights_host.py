"""Per-bin weights of the objective through the host layer: sots_match with "objectiveWeights" in type.HIP
(Evolutionary_Strategy_HIP makes the table for N and its sampleRate and applies it to the context and to the chunks in
flight, batched and queued alike)."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
sys.path.insert(0, os.path.join(ROOT, "tools"))
from track_overhead import targets  # noqa: E402

CHUNKS = 6
PER_CHUNK = ("Audio chunk", "Best parameters", "Best fitness", " p")
BAND = {"objectiveWeights": {"bandHz": [80, 6000]}}
# bins of N = 2048 at 44100 Hz inside 80 .. 6000 Hz: k = 4 (86.1 Hz) .. 278 (5986 Hz)
BAND_LINE = "Objective weights: bandHz 80 .. 6000, 275 of 1024 bins count\n"


def run_match(tmp_path, tag, hip_keys):
    """the shipped shape on noisy chunks from a float WAV file (the pattern of tests/test_gpu_objective_host.py)"""
    exe = os.path.join(PKG_DIR, "sots_match")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    audio = targets(CHUNKS, 2048).reshape(-1)
    audio = (audio / np.abs(audio).max() * 0.9).astype(np.float32)
    wav = tmp_path / "in.wav"
    with open(wav, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + audio.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3, 1, 44100, 44100 * 4, 4, 32))
        f.write(b"data" + struct.pack("<I", audio.nbytes) + audio.tobytes())
    cfg = json.load(open(os.path.join(PKG_DIR, "parameters.json")))
    cfg["general"].update({"isDebug": True, "isBenchmarking": False})
    cfg["audio"]["audioLengthLog2"] = 11
    cfg["evolutionary"].update({"numParents": 16, "numOffspring": 16, "numDimensions": 6, "numGenerations": 60,
                                "paramMins": [0.0] * 6, "paramMaxs": [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0]})
    cfg["type"]["HIP"].update({"synth": "3op_series", "workgroupSize": 32})
    cfg["type"]["HIP"].update(hip_keys)
    cfg["type"].update({"input": "audio", "audio": str(wav)})
    cfg["general"]["outputAudioPath"] = str(tmp_path / f"out_{tag}.wav")
    p = tmp_path / f"parameters_{tag}.json"
    p.write_text(json.dumps(cfg))
    return subprocess.run([exe, "-j", str(p)], capture_output=True, text=True, timeout=300, cwd=tmp_path)


def chunk_lines(out):
    lines = [l for l in out.stdout.splitlines() if l.startswith(PER_CHUNK + ("Overall best",))]
    return lines[:next(i for i, l in enumerate(lines) if l.startswith("Overall best"))]


def test_sequential_batched_and_queued_print_the_same_chunks(tmp_path):
    outs = []
    for tag, keys in (("one", {"chunksInFlight": 1}), ("batch", {"chunksInFlight": 4}), ("queue", {"chunksInFlight": 4, "chunkQueue": True})):
        out = run_match(tmp_path, tag, dict(keys, **BAND))
        assert out.returncode == 0, out.stderr
        assert out.stdout.count(BAND_LINE) == 1, out.stdout[:2000]
        outs.append(chunk_lines(out))
    assert len([l for l in outs[0] if l.startswith("Best fitness")]) == CHUNKS
    assert outs[0] == outs[1] == outs[2]
    # other weights, another search: not the lines of the unweighted run, which does not mention weights at all
    plain = run_match(tmp_path, "plain", {"chunksInFlight": 1})
    assert plain.returncode == 0, plain.stderr
    assert "Objective weights" not in plain.stdout
    assert chunk_lines(plain) != outs[0]


def test_weights_combine_with_the_log_objective(tmp_path):
    keys = {"objective": "logMagnitude", "objectiveFloor": 1e-3, "objectiveWeights": "aWeighting"}
    outs = []
    for tag, more in (("one", {"chunksInFlight": 1}), ("queue", {"chunksInFlight": 4, "chunkQueue": True})):
        out = run_match(tmp_path, tag, dict(keys, **more))
        assert out.returncode == 0, out.stderr
        assert out.stdout.count("Objective weights: aWeighting, 1023 of 1024 bins count\n") == 1
        outs.append(chunk_lines(out))
    assert outs[0] == outs[1]


def test_bad_keys_are_refused_before_any_device_work(tmp_path):
    table = [1.0] * 1024
    for value, text in (({"bandHz": [6000, 80]}, "bandHz needs 0 <= lo < hi"), ({"bandHz": [1, 20]}, "bandHz holds no bin"),
                        (table[:1000], "needs 1024 entries (N/2), got 1000"), ([-1.0] + table[1:], "entry 0 must be finite and not negative"),
                        ([0.0] * 1024, "at least one weight must be positive"), ("bWeighting", 'not "bWeighting"')):
        out = run_match(tmp_path, "bad", {"objectiveWeights": value})
        assert out.returncode != 0 and text in out.stderr, (value, out.stderr)
        assert "Audio chunk" not in out.stdout
