"""The phase-continuous rendering of the operator-graph voice through the host layer: sots_match with "synth": "graph", a
"voiceGraph" and "renderMode": "graphContinuous" / "graphContinuousGlide" in type.HIP.  The WAV it writes must be the NumPy
model's rendering (tests/_render_graph_continuous_model.py) of the parameter track it writes, after the writer's own 24-bit
quantisation; without "renderMatch" the key changes nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_graph_continuous_model as GM  # noqa: E402
import _render_model as M  # noqa: E402
from _graph_voice_match import CHAIN3, N, PMAX3, run_match  # noqa: E402
from test_gpu_render_host import read_wav24, stable  # noqa: E402

pytestmark = pytest.mark.gpu

HOP = N // 4
CHUNKS = (2 * N - N) // HOP + 1  # the input of _graph_voice_match is 2 N samples long
GRAPH = {"synth": "graph", "voiceGraph": CHAIN3, "chunksInFlight": 2, "hopSize": HOP}


def track_of(csv):
    cells = [l.split(",") for l in csv.read_text().splitlines()[1:]]
    return np.array([[float(x) for x in c[4:10]] for c in cells]).astype(np.float32)


@pytest.mark.parametrize("mode,glide", [("graphContinuous", False), ("graphContinuousGlide", True)])
def test_render_mode_writes_the_models_rendering_of_the_track(tmp_path, O, mode, glide):
    csv = tmp_path / "track.csv"
    out, wav = run_match(tmp_path, mode, dict(GRAPH, renderMatch=True, renderMode=mode, matchPath=str(csv)))
    assert out.returncode == 0, out.stderr
    u = track_of(csv)
    assert u.shape == (CHUNKS, 6)
    got = read_wav24(wav)
    assert len(got) == (CHUNKS - 1) * HOP + N
    want = M.quantise_24bit(GM.render(GM.GRAPHS["chain3"], None, u, [0.0] * 6, PMAX3, O.wavetable(), N, HOP, glide))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d samples differ" % np.count_nonzero(got != want)


def test_waveforms_reach_the_rendering(tmp_path, O):
    csv = tmp_path / "track.csv"
    names = ["half", "saw", "abs"]
    keys = dict(GRAPH, voiceWaveforms=names, renderMatch=True, renderMode="graphContinuous", matchPath=str(csv))
    out, wav = run_match(tmp_path, "waves", keys)
    assert out.returncode == 0, out.stderr
    want = M.quantise_24bit(GM.render(GM.GRAPHS["chain3"], [1, 7, 2], track_of(csv), [0.0] * 6, PMAX3, O.wavetable(), N, HOP, False))
    got = read_wav24(wav)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%d samples differ" % np.count_nonzero(got != want)


def test_the_mode_changes_the_rendering_and_nothing_else(tmp_path):
    keys = dict(GRAPH, renderMatch=True)
    plain, wav_plain = run_match(tmp_path, "plain", keys)
    cont, wav_cont = run_match(tmp_path, "cont", dict(keys, renderMode="graphContinuous"))
    assert plain.returncode == 0 and cont.returncode == 0, plain.stderr + cont.stderr
    assert stable(plain.stdout) == stable(cont.stdout)
    assert wav_plain.read_bytes() != wav_cont.read_bytes() and len(wav_plain.read_bytes()) == len(wav_cont.read_bytes())


def test_the_key_takes_effect_only_with_render_match(tmp_path):
    # 2^14 samples of the last chunk's match, as ever
    off, wav_off = run_match(tmp_path, "off", dict(GRAPH, renderMode="graphContinuousGlide"))
    ref, wav_ref = run_match(tmp_path, "ref", dict(GRAPH))
    assert off.returncode == 0 and ref.returncode == 0, off.stderr + ref.stderr
    assert wav_off.read_bytes() == wav_ref.read_bytes() and len(wav_off.read_bytes()) == 44 + 3 * (1 << 14)
    assert stable(off.stdout) == stable(ref.stdout)


def test_match_report_scores_the_continuous_rendering(tmp_path):
    report = tmp_path / "report.csv"
    keys = dict(GRAPH, chunkQueue=True, renderMatch=True, renderMode="graphContinuousGlide", matchReport=str(report))
    out, wav = run_match(tmp_path, "report", keys)
    assert out.returncode == 0, out.stderr
    rows = report.read_text().splitlines()
    assert rows[0] == "chunk,fitness,rendered_fitness" and len(rows) == 1 + CHUNKS
    values = np.array([[float(x) for x in r.split(",")[1:]] for r in rows[1:]])
    assert np.isfinite(values).all() and (values >= 0).all()
