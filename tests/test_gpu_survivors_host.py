"""Elitist survival through the host layer: sots_match with "survivors" in type.HIP (Evolutionary_Strategy_HIP applies it
to the context, to every island and to the chunks in flight, batched and queued alike)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from _survivors_model import PMAX, targets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
CHUNKS = 6


def run_match(tmp_path, tag, hip_keys):
    """the shipped shape on noisy chunks from a float WAV file (the pattern of tests/test_gpu_run_record.py)"""
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
                                "paramMins": [0.0] * 6, "paramMaxs": PMAX[1]})
    cfg["type"]["HIP"].update({"synth": "3op_series", "workgroupSize": 32})
    cfg["type"]["HIP"].update(hip_keys)
    cfg["type"].update({"input": "audio", "audio": str(wav)})
    cfg["general"]["outputAudioPath"] = str(tmp_path / f"out_{tag}.wav")
    p = tmp_path / f"parameters_{tag}.json"
    p.write_text(json.dumps(cfg))
    return subprocess.run([exe, "-j", str(p)], capture_output=True, text=True, timeout=300, cwd=tmp_path)


def test_history_best_column_never_rises(tmp_path):
    csv = tmp_path / "history.csv"
    out = run_match(tmp_path, "history", {"survivors": 1, "historyEvery": 1, "historyPath": str(csv)})
    assert out.returncode == 0, out.stderr
    lines = csv.read_text().splitlines()
    assert lines[0].startswith("chunk,generation,best,best_ever,")
    best = {}
    for l in lines[1:]:
        c = l.split(",")
        best.setdefault(int(c[0]), []).append(float(c[2]))
    assert sorted(best) == list(range(CHUNKS))
    for chunk, b in best.items():
        assert len(b) == 60
        assert all(y <= x for x, y in zip(b, b[1:])), (chunk, b)


def test_queue_prints_the_same_best_parameters(tmp_path):
    per_chunk = ("Audio chunk", "Best parameters", "Best fitness", " p")
    outs = []
    for tag, keys in (("one", {"chunksInFlight": 1}), ("queue", {"chunksInFlight": 4, "chunkQueue": True})):
        out = run_match(tmp_path, tag, dict(keys, survivors=1))
        assert out.returncode == 0, out.stderr
        lines = [l for l in out.stdout.splitlines() if l.startswith(per_chunk + ("Overall best",))]
        outs.append(lines[:next(i for i, l in enumerate(lines) if l.startswith("Overall best"))])
    assert len([l for l in outs[0] if l.startswith("Best fitness")]) == CHUNKS
    assert outs[0] == outs[1]


def test_too_many_survivors_are_refused_with_the_library_text(tmp_path):
    out = run_match(tmp_path, "bad", {"survivors": 17})
    assert out.returncode != 0
    assert "17 survivors asked for, at most numParents = 16 can be kept" in out.stderr
    # a count no population can hold reaches the library as the largest one; a negative one is refused by the reader
    out = run_match(tmp_path, "huge", {"survivors": 1e12})
    assert out.returncode != 0 and "4294967295 survivors asked for, at most numParents = 16" in out.stderr
    out = run_match(tmp_path, "negative", {"survivors": -1})
    assert out.returncode != 0 and "survivors must not be negative" in out.stderr
