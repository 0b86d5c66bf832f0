"""The spectral objective through the host layer: sots_match with "objective" / "objectiveFloor" in type.HIP
(Evolutionary_Strategy_HIP applies them to the context and to the chunks in flight, batched and queued alike)."""
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


def run_match(tmp_path, tag, hip_keys):
    """the shipped shape on noisy chunks from a float WAV file (the pattern of tests/test_gpu_survivors_host.py)"""
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


def without_times(text):
    """the driver's output without the lines that hold wall-clock figures (the driver's three and the Benchmarker's totals and average)"""
    timed = ("Total time to complete", "Average time to complete each buffer", "Candidates evaluated per second", "Chunks matched per second")
    return [l for l in text.splitlines() if not l.startswith(timed)]


def test_sequential_batched_and_queued_print_the_same_chunks(tmp_path):
    log = {"objective": "logMagnitude", "objectiveFloor": 1e-3}
    outs = []
    for tag, keys in (("one", {"chunksInFlight": 1}), ("batch", {"chunksInFlight": 4}), ("queue", {"chunksInFlight": 4, "chunkQueue": True})):
        out = run_match(tmp_path, tag, dict(keys, **log))
        assert out.returncode == 0, out.stderr
        assert out.stdout.count("Objective: logMagnitude, floor 0.001\n") == 1
        outs.append(chunk_lines(out))
    assert len([l for l in outs[0] if l.startswith("Best fitness")]) == CHUNKS
    assert outs[0] == outs[1] == outs[2]
    # another objective, another search: not the lines of the magnitude run
    plain = run_match(tmp_path, "plain", {"chunksInFlight": 1})
    assert plain.returncode == 0, plain.stderr
    assert chunk_lines(plain) != outs[0]


def test_without_the_keys_nothing_is_added(tmp_path):
    """the same binary with "magnitude" given explicitly prints the run without the keys plus the one line"""
    plain = run_match(tmp_path, "plain", {})
    named = run_match(tmp_path, "named", {"objective": "magnitude"})
    assert plain.returncode == 0 and named.returncode == 0, plain.stderr + named.stderr
    assert "Objective" not in plain.stdout
    a, b = without_times(plain.stdout), without_times(named.stdout)
    assert b.count("Objective: magnitude, floor 0") == 1
    b.remove("Objective: magnitude, floor 0")
    assert a == b


def test_bad_keys_are_refused_before_any_device_work(tmp_path):
    for keys, text in (({"objective": "mel", "objectiveFloor": 1e-3}, 'not "mel"'), ({"objective": "logMagnitude"}, "needs type.HIP.objectiveFloor"),
                       ({"objective": "logMagnitude", "objectiveFloor": 2.0}, "must lie in 1e-30 .. 1")):
        out = run_match(tmp_path, "bad", keys)
        assert out.returncode != 0 and text in out.stderr, (keys, out.stderr)
