"""The graph voice's per-operator feedback through the host layer: sots_match with "voiceFeedback" beside "voiceGraph" on the
two-chunk input of tests/_graph_voice_match.py - through the chunk queue and chunk by chunk, with the rendering of the whole
match - and, with "input": "params", the host's own synthesiser against the model."""
import json
import os
import subprocess

import numpy as np
import pytest

import _render_model as R
from _graph_feedback_model import GRAPHS, graph_synth_feedback, graph_synth_waves
from _graph_voice_match import CHAIN3, GENS, N, PKG_DIR, PMAX3, run_match

pytestmark = pytest.mark.gpu

CODES = [0, 7, 0]
BETA = [0.5, 0.0, 1.0]
GRAPH = {"synth": "graph", "voiceGraph": CHAIN3, "voiceWaveforms": ["sine", "saw", "sine"], "voiceFeedback": [0.5, 0, 1]}


def samples_24bit(path):
    data = np.frombuffer(open(path, "rb").read()[44:], np.uint8).reshape(-1, 3).astype(np.int32)
    value = data[:, 0] | data[:, 1] << 8 | data[:, 2] << 16
    value = np.where(value >= 1 << 23, value - (1 << 24), value)
    return (value / 8388608.0).astype(np.float32)


def track_genes(csv):
    return np.array([[float(x) for x in l.split(",")[4:10]] for l in csv.read_text().splitlines()[1:]]).astype(np.float32)


def test_the_rendered_rows_are_the_models_through_the_queue_and_chunk_by_chunk(tmp_path, O):
    """renderMatch at hop N: the chunks' best parameters synthesised with the feedback, end to end - the model's audio of the
    track's unit-range genes, through the 24-bit file"""
    results = []
    for tag, keys in (("queue", {"chunksInFlight": 2, "chunkQueue": True}), ("one", {"chunksInFlight": 1})):
        csv = tmp_path / f"track_{tag}.csv"
        out, wav = run_match(tmp_path, tag, dict(GRAPH, **keys, renderMatch=True, matchPath=str(csv)))
        assert out.returncode == 0, out.stderr
        assert wav.exists() and len(wav.read_bytes()) == 44 + 3 * 2 * N
        cells = [l.split(",") for l in csv.read_text().splitlines()[1:]]
        assert len(cells) == 2 and all(len(c) == 4 + 12 and int(c[2]) == GENS for c in cells)
        want = graph_synth_feedback(GRAPHS["chain3"], CODES, BETA, track_genes(csv), [0.0] * 6, PMAX3, N, O.wavetable()).reshape(-1)
        assert np.array_equal(samples_24bit(wav), R.quantise_24bit(want)), tag
        results.append((csv.read_bytes(), wav.read_bytes()))
    assert results[0] == results[1], "queue and chunk by chunk differ"
    # the setting reached the search: the run without it finds another track
    off_csv = tmp_path / "track_off.csv"
    keys = {k: v for k, v in GRAPH.items() if k != "voiceFeedback"}
    out, _ = run_match(tmp_path, "off", dict(keys, chunksInFlight=2, chunkQueue=True, matchPath=str(off_csv)))
    assert out.returncode == 0 and off_csv.read_bytes() != results[0][0]


def test_without_render_match_the_host_synthesiser_writes_the_last_match(tmp_path, O):
    csv = tmp_path / "track.csv"
    out, wav = run_match(tmp_path, "plain", dict(GRAPH, chunksInFlight=1, matchPath=str(csv)))
    assert out.returncode == 0, out.stderr
    want = graph_synth_feedback(GRAPHS["chain3"], CODES, BETA, track_genes(csv)[-1:], [0.0] * 6, PMAX3, 1 << 14, O.wavetable())[0]
    assert np.array_equal(samples_24bit(wav), R.quantise_24bit(want))


def test_with_input_params_the_hosts_target_is_the_model(tmp_path, O):
    cfg = json.load(open(os.path.join(PKG_DIR, "parameters.json")))
    cfg["general"].update({"isDebug": True, "isBenchmarking": False, "outputAudioPath": str(tmp_path / "out.wav")})
    cfg["audio"]["audioLengthLog2"] = 10
    params = [1450.0, 3.0, 210.0, 2.5, 440.0, 0.75]
    cfg["evolutionary"].update({"numParents": 32, "numOffspring": 32, "numDimensions": 6, "numGenerations": 5,
                                "paramMins": [0.0] * 6, "paramMaxs": PMAX3})
    cfg["type"]["HIP"].update(dict(GRAPH, workgroupSize=32))
    cfg["type"].update({"input": "params", "params": params})
    p = tmp_path / "parameters.json"
    p.write_text(json.dumps(cfg))
    out = subprocess.run([os.path.join(PKG_DIR, "sots_match"), "-j", str(p)], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert out.returncode == 0, out.stderr
    lo, hi = np.zeros(6, np.float32), np.asarray(PMAX3, np.float32)
    unit = (np.asarray(params, np.float32) - lo) / (hi - lo)
    want = graph_synth_feedback(GRAPHS["chain3"], CODES, BETA, unit[None, :], [0.0] * 6, PMAX3, N, O.wavetable())[0]
    assert np.array_equal(samples_24bit(tmp_path / "inputGenerated.wav"), R.quantise_24bit(want))
    off = graph_synth_waves(GRAPHS["chain3"], CODES, unit[None, :], [0.0] * 6, PMAX3, N, O.wavetable())[0]
    assert not np.array_equal(R.quantise_24bit(want), R.quantise_24bit(off))
