"""Feedback indices as genes through the host layer: sots_match with "voiceFeedbackGenes" beside "voiceGraph" on the
two-chunk input of tests/_graph_voice_match.py - through the chunk queue and chunk by chunk, with the rendering of the whole
match and the parameter track, whose rows carry the index - and the host's own synthesiser against the model."""
import numpy as np
import pytest

import _render_model as R
from _graph_feedback_genes_model import GRAPHS, graph_synth_genes
from _graph_voice_match import CHAIN3, GENS, N, PMAX3, run_match

pytestmark = pytest.mark.gpu

CODES = [0, 7, 0]
BETA = [0.5, 0.0, 0.0]  # operator 0 keeps a fixed index; operator 2's is the gene
MASK = 0b100
PMAX = PMAX3 + [2.0]
GRAPH = {"synth": "graph", "voiceGraph": CHAIN3, "voiceWaveforms": ["sine", "saw", "sine"], "voiceFeedback": [0.5, 0, 0], "voiceFeedbackGenes": [0, 0, 1]}


def samples_24bit(path):
    data = np.frombuffer(open(path, "rb").read()[44:], np.uint8).reshape(-1, 3).astype(np.int32)
    value = data[:, 0] | data[:, 1] << 8 | data[:, 2] << 16
    value = np.where(value >= 1 << 23, value - (1 << 24), value)
    return (value / 8388608.0).astype(np.float32)


def track_genes(csv):
    return np.array([[float(x) for x in l.split(",")[4:11]] for l in csv.read_text().splitlines()[1:]]).astype(np.float32)


def test_the_rendered_rows_are_the_models_through_the_queue_and_chunk_by_chunk(tmp_path, O):
    """renderMatch at hop N: every chunk's best row synthesised with ITS index, end to end, through the 24-bit file; the
    track has seven unit-range and seven scaled columns"""
    results = []
    for tag, keys in (("queue", {"chunksInFlight": 2, "chunkQueue": True}), ("one", {"chunksInFlight": 1})):
        csv = tmp_path / f"track_{tag}.csv"
        out, wav = run_match(tmp_path, tag, dict(GRAPH, **keys, renderMatch=True, matchPath=str(csv)), dims=7, pmax=PMAX)
        assert out.returncode == 0, out.stderr
        assert wav.exists() and len(wav.read_bytes()) == 44 + 3 * 2 * N
        cells = [l.split(",") for l in csv.read_text().splitlines()[1:]]
        assert len(cells) == 2 and all(len(c) == 4 + 14 and int(c[2]) == GENS for c in cells)
        want = graph_synth_genes(GRAPHS["chain3"], CODES, BETA, MASK, track_genes(csv), [0.0] * 7, PMAX, N, O.wavetable()).reshape(-1)
        assert np.array_equal(samples_24bit(wav), R.quantise_24bit(want)), tag
        results.append((csv.read_bytes(), wav.read_bytes()))
    assert results[0] == results[1], "queue and chunk by chunk differ"


def test_without_render_match_the_host_synthesiser_writes_the_last_match(tmp_path, O):
    csv = tmp_path / "track.csv"
    out, wav = run_match(tmp_path, "plain", dict(GRAPH, chunksInFlight=1, matchPath=str(csv)), dims=7, pmax=PMAX)
    assert out.returncode == 0, out.stderr
    want = graph_synth_genes(GRAPHS["chain3"], CODES, BETA, MASK, track_genes(csv)[-1:], [0.0] * 7, PMAX, 1 << 14, O.wavetable())[0]
    assert np.array_equal(samples_24bit(wav), R.quantise_24bit(want))
