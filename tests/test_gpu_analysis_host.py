"""Analysis on the device through the host layer: sots_match with "deviceAnalysis" and "matchReport" in
type.HIP, on 8 chunks of the SHORT shape (2-op, N = 256, P = 32) through the chunk queue with one survivor, the whole match
rendered as one continuous voice (parameters held)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from _carry_model import gliding_track

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
PMAX = [3520.0, 8.0, 3520.0, 1.0]
N, HOP, CHUNKS, GENS = 256, 64, 8, 20
BASE = {"chunksInFlight": 4, "chunkQueue": True, "survivors": 1, "hopSize": HOP, "renderMatch": True, "renderMode": "continuous"}


def run_match(tmp_path, tag, hip_keys, env=None):
    exe = os.path.join(PKG_DIR, "sots_match")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    audio = (0.9 * gliding_track(CHUNKS, N, HOP)).astype(np.float32)
    wav = tmp_path / "in.wav"
    with open(wav, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + audio.nbytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3, 1, 44100, 44100 * 4, 4, 32))
        f.write(b"data" + struct.pack("<I", audio.nbytes) + audio.tobytes())
    cfg = json.load(open(os.path.join(PKG_DIR, "parameters.json")))
    cfg["general"].update({"isDebug": True, "isBenchmarking": False})
    cfg["audio"]["audioLengthLog2"] = 8
    cfg["evolutionary"].update({"numParents": 16, "numOffspring": 16, "numDimensions": 4, "numGenerations": GENS,
                                "paramMins": [0.0] * 4, "paramMaxs": PMAX})
    cfg["type"]["HIP"].update({"synth": "2op", "workgroupSize": 32})
    cfg["type"]["HIP"].update(hip_keys)
    cfg["type"].update({"input": "audio", "audio": str(wav)})
    out_wav = tmp_path / f"out_{tag}.wav"
    cfg["general"]["outputAudioPath"] = str(out_wav)
    p = tmp_path / f"parameters_{tag}.json"
    p.write_text(json.dumps(cfg))
    run_env = dict(os.environ)
    run_env.update(env or {})
    return subprocess.run([exe, "-j", str(p)], capture_output=True, text=True, timeout=300, cwd=tmp_path, env=run_env), out_wav


def stable(stdout):
    """the lines of results (none of the wall-clock figures)"""
    return [l for l in stdout.splitlines() if l.startswith(("Audio chunk", "Best parameters", "Best fitness", " p", "Overall best", " Fitness"))]


def printed_fitness(stdout):
    return [l.split(": ")[1] for l in stdout.splitlines() if l.startswith("Best fitness")]


def test_device_analysis_matches_and_writes_a_track(tmp_path):
    csv = tmp_path / "track.csv"
    out, wav = run_match(tmp_path, "device", dict(BASE, deviceAnalysis=True, matchPath=str(csv)))
    assert out.returncode == 0, out.stderr
    rows = csv.read_text().splitlines()
    assert len(rows) - 1 == CHUNKS
    fit = np.array([float(r.split(",")[3]) for r in rows[1:]])
    assert np.isfinite(fit).all() and (fit >= 0).all()
    assert len(wav.read_bytes()) == 44 + 3 * ((CHUNKS - 1) * HOP + N)
    # the host analysis of the same run: the same number of lines, not the same bits (fp32 against fp64 targets)
    host, _ = run_match(tmp_path, "host", dict(BASE, matchPath=str(tmp_path / "track_host.csv")))
    assert host.returncode == 0, host.stderr
    assert len(stable(host.stdout)) == len(stable(out.stdout))
    # ... and in flight without the queue
    flight, _ = run_match(tmp_path, "flight", dict(BASE, chunkQueue=False, deviceAnalysis=True, matchPath=str(tmp_path / "track_flight.csv")))
    assert flight.returncode == 0, flight.stderr
    assert (tmp_path / "track_flight.csv").read_bytes() == csv.read_bytes()   # (the queue and the batches report the same chunks)


@pytest.mark.parametrize("device", [False, True])
def test_match_report_rows(tmp_path, device):
    report = tmp_path / "report.csv"
    out, wav_report = run_match(tmp_path, "report", dict(BASE, deviceAnalysis=device, matchReport=str(report)))
    assert out.returncode == 0, out.stderr
    lines = report.read_text().splitlines()
    assert lines[0] == "chunk,fitness,rendered_fitness" and len(lines) - 1 == CHUNKS
    cells = [l.split(",") for l in lines[1:]]
    assert [int(c[0]) for c in cells] == list(range(CHUNKS))
    values = np.array([[float(c[1]), float(c[2])] for c in cells])
    assert np.isfinite(values).all() and (values >= 0).all()
    assert ["%g" % np.float32(c[1]) for c in cells] == printed_fitness(out.stdout)   # column 2: the fitness the match printed
    # nothing else changed: the same run without the report prints and renders the same
    plain, wav_plain = run_match(tmp_path, "plain", dict(BASE, deviceAnalysis=device))
    assert stable(plain.stdout) == stable(out.stdout) and wav_plain.read_bytes() == wav_report.read_bytes()


def test_without_the_keys_nothing_changes(tmp_path):
    csv_a, csv_b = tmp_path / "a.csv", tmp_path / "b.csv"
    absent, wav_a = run_match(tmp_path, "absent", dict(BASE, matchPath=str(csv_a)))
    off, wav_b = run_match(tmp_path, "off", dict(BASE, deviceAnalysis=False, matchPath=str(csv_b)))
    assert absent.returncode == 0 and off.returncode == 0, absent.stderr + off.stderr

    def without_times(text):   # every line but the wall-clock figures, which no two runs share
        return [l for l in text.splitlines() if not l.startswith(("Total time", "Average time", "Candidates evaluated", "Chunks matched"))]

    assert without_times(absent.stdout) == without_times(off.stdout)
    assert absent.stderr == off.stderr
    assert csv_a.read_bytes() == csv_b.read_bytes() and wav_a.read_bytes() == wav_b.read_bytes()
    assert not any(n.startswith("report") for n in os.listdir(tmp_path))
