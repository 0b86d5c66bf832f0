"""The operator-graph voice through the host layer: sots_match with "synth": "graph" and "voiceGraph" on a two-chunk input,
through the chunk queue and chunk by chunk - the parameter track has 2 x operators gene columns, the rendering is written,
the report scores it, and both paths print and write the same."""
import numpy as np
import pytest

from _graph_voice_match import CHAIN3, GENS, N, PMAX3, run_match

pytestmark = pytest.mark.gpu

GRAPH = {"synth": "graph", "voiceGraph": CHAIN3}


def stable(stdout):
    """the lines of results (none of the wall-clock figures)"""
    return [l for l in stdout.splitlines() if l.startswith(("Audio chunk", "Best parameters", "Best fitness", " p", "Overall best", " Fitness"))]


def test_queue_and_chunk_by_chunk_match_two_chunks_with_a_voice_graph(tmp_path):
    results = []
    for tag, keys in (("queue", {"chunksInFlight": 2, "chunkQueue": True}), ("one", {"chunksInFlight": 1})):
        csv = tmp_path / f"track_{tag}.csv"
        out, wav = run_match(tmp_path, tag, dict(GRAPH, **keys, renderMatch=True, matchPath=str(csv)))
        assert out.returncode == 0, out.stderr
        assert wav.exists() and len(wav.read_bytes()) == 44 + 3 * 2 * N  # 24-bit samples of both chunks, end to end
        results.append((csv.read_bytes(), wav.read_bytes(), out.stdout))
    assert results[0][0] == results[1][0], "the parameter tracks differ"
    assert results[0][1] == results[1][1], "the renderings differ"
    assert stable(results[0][2]) == stable(results[1][2])

    lines = results[0][0].decode().splitlines()
    assert lines[0] == "chunk,start_sample,generations,fitness," + ",".join(f"u{i}" for i in range(6)) + "," + ",".join(f"p{i}" for i in range(6))
    cells = [l.split(",") for l in lines[1:]]
    assert len(cells) == 2 and all(len(c) == 4 + 12 and int(c[2]) == GENS for c in cells)
    u = np.array([[float(x) for x in c[4:10]] for c in cells]).astype(np.float32)
    p = np.array([[float(x) for x in c[10:16]] for c in cells]).astype(np.float32)
    assert np.all((u >= 0) & (u <= 1))
    np.testing.assert_allclose(p, u * np.array(PMAX3, np.float32), rtol=1e-6)


def test_match_report_and_the_last_chunk_rendering(tmp_path):
    report = tmp_path / "report.csv"
    out, wav = run_match(tmp_path, "report", dict(GRAPH, chunksInFlight=2, chunkQueue=True, renderMatch=True, matchReport=str(report)))
    assert out.returncode == 0, out.stderr
    rows = report.read_text().splitlines()
    assert rows[0] == "chunk,fitness,rendered_fitness" and len(rows) == 3
    values = np.array([[float(x) for x in r.split(",")[1:]] for r in rows[1:]])
    assert np.isfinite(values).all() and (values >= 0).all()
    # without renderMatch: 2^14 samples of the last chunk's match from the host's own graph synthesiser
    out, wav = run_match(tmp_path, "plain", dict(GRAPH, chunksInFlight=2))
    assert out.returncode == 0, out.stderr
    assert len(wav.read_bytes()) == 44 + 3 * (1 << 14)
    assert sum(l.startswith(" p") for l in out.stdout.splitlines()) >= 6
