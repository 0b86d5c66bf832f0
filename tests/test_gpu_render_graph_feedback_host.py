"""The phase-continuous rendering of a graph voice with feedback through the host layer: sots_match with "synth": "graph", a
"voiceGraph", a "voiceFeedback" and "renderMode": "graphFeedback" / "graphFeedbackGlide" in type.HIP.  The WAV it writes must
be the NumPy model's rendering (tests/_render_graph_feedback_model.py) of the parameter track it writes, after the writer's own
24-bit quantisation; without "renderMatch" the key changes nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_graph_feedback_model as RM  # noqa: E402
import _render_model as M  # noqa: E402
from _graph_voice_match import CHAIN3, N, PMAX3, run_match  # noqa: E402
from test_gpu_render_graph_continuous_host import CHUNKS, HOP, track_of  # noqa: E402
from test_gpu_render_host import read_wav24, stable  # noqa: E402

pytestmark = pytest.mark.gpu

BETA = [0.0, 0.5, 0.75]
GRAPH = {"synth": "graph", "voiceGraph": CHAIN3, "voiceFeedback": BETA, "chunksInFlight": 2, "hopSize": HOP}


@pytest.mark.parametrize("mode,glide", [("graphFeedback", False), ("graphFeedbackGlide", True)])
def test_render_mode_writes_the_models_rendering_of_the_track(tmp_path, O, mode, glide):
    csv = tmp_path / "track.csv"
    out, wav = run_match(tmp_path, mode, dict(GRAPH, renderMatch=True, renderMode=mode, matchPath=str(csv)))
    assert out.returncode == 0, out.stderr
    u = track_of(csv)
    assert u.shape == (CHUNKS, 6)
    got = read_wav24(wav)
    assert len(got) == (CHUNKS - 1) * HOP + N
    want = M.quantise_24bit(RM.render(RM.GRAPHS["chain3"], None, BETA, u, [0.0] * 6, PMAX3, O.wavetable(), N, HOP, glide, form="relax"))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d samples differ" % np.count_nonzero(got != want)


def test_the_key_takes_effect_only_with_render_match(tmp_path):
    # 2^14 samples of the last chunk's match, as ever
    off, wav_off = run_match(tmp_path, "off", dict(GRAPH, renderMode="graphFeedbackGlide"))
    ref, wav_ref = run_match(tmp_path, "ref", dict(GRAPH))
    assert off.returncode == 0 and ref.returncode == 0, off.stderr + ref.stderr
    assert wav_off.read_bytes() == wav_ref.read_bytes() and len(wav_off.read_bytes()) == 44 + 3 * (1 << 14)
    assert stable(off.stdout) == stable(ref.stdout)
