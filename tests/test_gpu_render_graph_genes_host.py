"""The phase-continuous rendering of a graph voice whose feedback indices are genes through the host layer: sots_match with
"synth": "graph", the 2-op graph, "voiceFeedbackGenes": [0, 1] and "renderMode": "graphGenes" / "graphGenesGlide" in type.HIP,
at a hop of N/4.  The WAV it writes must be the NumPy model's rendering (tests/_render_graph_genes_model.py) of the parameter
track it writes - five genes a chunk, the carrier's feedback index the fifth - after the writer's own 24-bit quantisation."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_graph_genes_model as NM  # noqa: E402
import _render_model as M  # noqa: E402
from _graph_voice_match import N, run_match  # noqa: E402
from test_gpu_render_host import read_wav24  # noqa: E402

pytestmark = pytest.mark.gpu

HOP = N // 4
CHUNKS = (2 * N - N) // HOP + 1  # the input of _graph_voice_match is 2 N samples long
TWO_OP = {"operators": 2, "modulators": [[], [0]], "carriers": [1]}
PMAX = [3520.0, 8.0, 3520.0, 1.0, 2.0]
KEYS = {"synth": "graph", "voiceGraph": TWO_OP, "voiceFeedbackGenes": [0, 1], "chunksInFlight": 2, "hopSize": HOP}


def track_of(csv, d):
    cells = [l.split(",") for l in csv.read_text().splitlines()[1:]]
    return np.array([[float(x) for x in c[4:4 + d]] for c in cells]).astype(np.float32)


@pytest.mark.parametrize("mode,glide", [("graphGenes", False), ("graphGenesGlide", True)])
def test_render_mode_writes_the_models_rendering_of_the_track(tmp_path, O, mode, glide):
    csv = tmp_path / "track.csv"
    out, wav = run_match(tmp_path, mode, dict(KEYS, renderMatch=True, renderMode=mode, matchPath=str(csv)), dims=5, pmax=PMAX)
    assert out.returncode == 0, out.stderr
    u = track_of(csv, 5)
    assert u.shape == (CHUNKS, 5)
    assert np.ptp(u[:, 4]) > 0, "the chunks' feedback genes differ: the index moves along the track"
    got = read_wav24(wav)
    assert len(got) == (CHUNKS - 1) * HOP + N
    want = M.quantise_24bit(NM.render(NM.GRAPHS["2op"], None, None, 0b10, u, [0.0] * 5, PMAX, O.wavetable(), N, HOP, glide, form="relax"))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d samples differ" % np.count_nonzero(got != want)
