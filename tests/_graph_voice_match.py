"""sots_match runs with the operator-graph voice, for tests/test_graph_voice_cpu.py (refusals that need no device) and
tests/test_gpu_graph_voice_host.py: a two-chunk WAV input and a parameters.json whose type.HIP block carries the keys."""
import json
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
N, GENS = 1024, 20
CHAIN3 = {"operators": 3, "modulators": [[], [0], [1]], "carriers": [2]}
PMAX3 = [3520.0, 8.0, 3520.0, 8.0, 3520.0, 1.0]
NO_DEVICE = {"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}


def signal(length=2 * N):
    t = np.arange(length) / 44100.0
    rng = np.random.default_rng(5)
    a = 0.6 * np.sin(2 * np.pi * 330.0 * t) + 0.3 * np.sin(2 * np.pi * 891.0 * t) + 0.05 * rng.standard_normal(length)
    return (a / np.abs(a).max() * 0.9).astype(np.float32)


def run_match(tmp_path, tag, hip_keys, dims=6, pmax=PMAX3, env=None):
    """(the finished process, the path of the WAV it was to write)"""
    exe = os.path.join(PKG_DIR, "sots_match")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    audio = signal()
    wav = tmp_path / "in.wav"
    with open(wav, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + audio.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3, 1, 44100, 44100 * 4, 4, 32))
        f.write(b"data" + struct.pack("<I", audio.nbytes) + audio.tobytes())
    cfg = json.load(open(os.path.join(PKG_DIR, "parameters.json")))
    cfg["general"].update({"isDebug": True, "isBenchmarking": False})
    cfg["audio"]["audioLengthLog2"] = 10
    cfg["evolutionary"].update({"numParents": 32, "numOffspring": 32, "numDimensions": dims, "numGenerations": GENS,
                                "paramMins": [0.0] * len(pmax), "paramMaxs": pmax})
    cfg["type"]["HIP"].update({"workgroupSize": 32})
    cfg["type"]["HIP"].update(hip_keys)
    cfg["type"].update({"input": "audio", "audio": str(wav)})
    out_wav = tmp_path / f"out_{tag}.wav"
    cfg["general"]["outputAudioPath"] = str(out_wav)
    p = tmp_path / f"parameters_{tag}.json"
    p.write_text(json.dumps(cfg))
    run_env = dict(os.environ)
    run_env.update(env or {})
    return subprocess.run([exe, "-j", str(p)], capture_output=True, text=True, timeout=300, cwd=tmp_path, env=run_env), out_wav
