"""CPU-side checks of the operator-graph voice (SOTS_SYNTH_GRAPH, sots_create_graph, sots_batch_create_graph): the NumPy
model of the definition (tests/_graph_voice_model.py) equals the oracle bit for bit on the two graphs that restate a fixed
voice, its vectorised and scalar forms agree, the rules are clean under ASan + UBSan in a stand-alone program
(tests/graph_rules_san.cpp; nothing is loaded into Python under a sanitizer), and every refusal that needs no device comes
back through the C-ABI with its code and text.  The refusals that need a context (device-kernel arithmetic, continuous
rendering) are driven at rule level by the stand-alone program here and through the C-ABI in tests/test_gpu_graph_voice.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _graph_voice_model import GRAPHS, edge_rows, graph_synth, graph_synth_scalar, overflow_ranges, ranges

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")


@pytest.fixture(scope="module")
def table(O):
    return O.wavetable()


# ---- the model against the oracle: the anchors ----
def anchor_rows(d, rows, seed):
    """rows in [0, 1] with all-0 and all-1 rows and single genes at 0 and at 1"""
    v = edge_rows(d, rows, seed)
    v[2, 0], v[3, 1], v[4, 2], v[5, 3] = 0.0, 1.0, 1.0, 0.0
    return v


@pytest.mark.parametrize("n", [256, 1024])
@pytest.mark.parametrize("negative", [False, True])
def test_2op_anchor_equals_the_oracle(O, table, n, negative):
    pmin = [-880.0, -2.0, -440.0, -1.0] if negative else [0.0] * 4
    pmax = [3520.0, 8.0, 3520.0, 1.0]
    v = anchor_rows(4, 12, 11 + n)
    got = graph_synth(GRAPHS["2op"], v, pmin, pmax, n, table)
    for r in range(v.shape[0]):
        want = O.synth(O.SYNTH_2OP, v[r], pmin, pmax, n, table)
        assert np.array_equal(got[r].view(np.uint32), want.view(np.uint32)), (r, n, negative)


@pytest.mark.parametrize("n", [256, 1024])
@pytest.mark.parametrize("negative", [False, True])
def test_triple_anchor_equals_the_oracle(O, table, n, negative):
    """the triple voice scales every pair by ranges 0..3: the graph's ranges repeat them per pair"""
    pmin = [-880.0, -2.0, -440.0, -1.0] if negative else [0.0] * 4
    pmax = [3520.0, 8.0, 3520.0, 1.0]
    v = anchor_rows(12, 8, 23 + n)
    got = graph_synth(GRAPHS["triple"], v, pmin * 3, pmax * 3, n, table)
    for r in range(v.shape[0]):
        want = O.synth(O.SYNTH_TRIPLE_PAR, v[r], pmin, pmax, n, table)
        assert np.array_equal(got[r].view(np.uint32), want.view(np.uint32)), (r, n, negative)


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_vectorised_model_equals_its_scalar_restatement(table, name):
    g = GRAPHS[name]
    pmin, pmax = ranges(g[0])
    v = edge_rows(2 * g[0], 5, 5)
    got = graph_synth(g, v, pmin, pmax, 256, table)
    for r in range(v.shape[0]):
        want = graph_synth_scalar(g, v[r], pmin, pmax, 256, table)
        assert np.array_equal(got[r].view(np.uint32), want.view(np.uint32)), (name, r)


def test_the_edge_ranges_reach_the_clamp_and_the_lower_wrap(table):
    """what the GPU test's ranges are for: phases below 0 and steps of more than W per sample do occur"""
    g = GRAPHS["2op"]
    pmin, pmax = ranges(2)
    p = np.asarray(pmin, np.float32) + edge_rows(4, 64, 3) * (np.asarray(pmax, np.float32) - np.asarray(pmin, np.float32))
    step = np.abs(p[:, 0] * p[:, 1]) * np.float32(32768 / 44100)
    assert (step > 2 * 32768).any() and (p[:, 2] < 0).any()
    assert np.isfinite(graph_synth(g, edge_rows(4, 64, 3), pmin, pmax, 256, table)).all()


def test_the_new_graphs_are_the_operator_counts_and_shapes_they_are_named_for():
    """OPS 4, 5 and 7 (the three forms of the kernel no older graph reaches), a fan-in of 6, eight carriers, a fan-out of 7"""
    assert {g[0] for g in GRAPHS.values()} == {2, 3, 4, 5, 6, 7, 8}
    assert (GRAPHS["fan3"][0], GRAPHS["stacks5"][0], GRAPHS["seven"][0]) == (4, 5, 7)
    assert GRAPHS["dense8"][1] == [0, 1, 3, 7, 15, 31, 63, 63] and max(bin(m).count("1") for m in GRAPHS["dense8"][1]) == 6
    assert bin(GRAPHS["additive8"][2]).count("1") == 8 and not any(GRAPHS["additive8"][1])
    assert sum(m & 1 for m in GRAPHS["one_to_seven"][1]) == 7


@pytest.mark.parametrize("name", ["fan3", "dense8"])
def test_the_overflow_ranges_make_infinite_and_nan_outputs_and_phases(table, name):
    """what the GPU test's overflow ranges are for: finite genes, yet modulator outputs that are inf and that are NaN and
    phases that are NaN do occur in the model - and the audio stays finite, since no carrier is overflowed.  (No phase is
    inf under these ranges: every phase starts at 0 and table[0] is 0, so an infinite level gives 0 x inf = NaN at sample 0
    and the phases it feeds are NaN from there on; the outputs are -inf from sample 1, where operator 0 reads entry W-1.)"""
    g = GRAPHS[name]
    pmin, pmax = overflow_ranges(g[0])
    v = edge_rows(2 * g[0], 96, 1256)  # the rows of the GPU case
    assert np.isfinite(v).all() and np.isfinite(pmin).all() and np.isfinite(pmax).all()
    seen = {}
    audio = graph_synth(g, v, pmin, pmax, 256, table, seen)
    assert table[0] == 0.0
    assert seen["output_inf"] and seen["output_nan"] and seen["phase_nan"], seen
    assert np.isfinite(audio).all() and np.abs(audio).max() > 0.01
    for r in (1, 2, 95):
        want = graph_synth_scalar(g, v[r], pmin, pmax, 256, table)
        assert np.array_equal(audio[r].view(np.uint32), want.view(np.uint32)), (name, r)


# ---- the rules, stand-alone, under the sanitizers ----
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_graph_rules_are_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "graph_rules_san"
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", *SAN, "-o", str(exe),
                           os.path.join(ROOT, "tests", "graph_rules_san.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert "graph rules: 36 checks, 0 failures" in out.stdout


# ---- refusals through the C-ABI that need no device ----
def test_new_symbols_and_struct(hip):
    lib = hip.load()
    for n in ("sots_create_graph", "sots_batch_create_graph", "sots_get_voice_graph"):
        assert n in hip.EXPORTS and hasattr(lib, n), n
    assert C.sizeof(hip.VoiceGraph) == 44 and hip.VoiceGraph.modulators.offset == 12
    assert hip.SYNTH_GRAPH == 4 and hip.SYNTH_NAMES["graph"] == 4
    assert hip.synth_dims(hip.SYNTH_GRAPH, hip.make_voice_graph(*GRAPHS["chain8"])) == 16
    assert hip.synth_dims(hip.SYNTH_TRIPLE_PAR) == 12
    with pytest.raises(ValueError):
        hip.synth_dims(hip.SYNTH_GRAPH)


def graph_cfg(hip, graph, **over):
    g = hip.make_voice_graph(*graph)
    cfg = hip.make_config(16, 16, hip.SYNTH_GRAPH, 10, None, [3520.0, 8.0] * g.num_operators, graph=g)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg, g


NEEDS_GRAPH = "synth_kind 4 (SOTS_SYNTH_GRAPH) needs its topology: sots_create_graph / sots_batch_create_graph"


def test_the_plain_entry_points_refuse_kind_4_and_name_the_graph_one(hip):
    lib = hip.load()
    cfg, _ = graph_cfg(hip, GRAPHS["2op"])
    h = C.c_void_p()
    assert lib.sots_create(C.byref(cfg), C.byref(h)) == -1 and not h.value
    assert lib.sots_last_error(None).decode() == NEEDS_GRAPH
    assert lib.sots_batch_create(C.byref(cfg), 2, C.byref(h)) == -1 and not h.value
    assert lib.sots_batch_last_error(None).decode() == NEEDS_GRAPH
    one = (C.c_int32 * 1)(0)
    assert lib.sots_group_create(C.byref(cfg), one, 1, 4, 1, 0, C.byref(h)) == -1 and not h.value
    assert lib.sots_group_last_error(None).decode() == "island 0: " + NEEDS_GRAPH


def test_kind_9_stays_unknown(hip):
    lib = hip.load()
    cfg, g = graph_cfg(hip, GRAPHS["2op"], synth_kind=9)
    h = C.c_void_p()
    assert lib.sots_create(C.byref(cfg), C.byref(h)) == -1
    assert lib.sots_last_error(None).decode() == "unknown synth_kind 9"
    assert lib.sots_create_graph(C.byref(cfg), C.byref(g), C.byref(h)) == -1
    assert lib.sots_last_error(None).decode() == "a voice graph needs synth_kind 4 (SOTS_SYNTH_GRAPH), got 9"


MALFORMED = [
    ((1, [0], 1), {}, "voice graph: 1 operators outside 2..8"),
    ((9, [0] * 8, 1), {}, "voice graph: 9 operators outside 2..8"),
    ((3, [0, 0b11, 0b10], 0b100), {}, "voice graph: modulators[1] = 0x3 has a bit at or above 1 (feed-forward only: operator i < j modulates j)"),
    ((3, [0, 0b1, 0b1], 0b100), {}, "voice graph: operator 1 is dead: neither a carrier nor a modulator"),
    ((3, [0, 0b1, 0b10], 0b110), {}, "voice graph: operator 1 is a carrier and modulates (one or the other)"),
    ((2, [0, 0b1], 0), {}, "voice graph: no carrier"),
    ((2, [0, 0b1], 0b110), {}, "voice graph: carriers 0x6 has bits beyond operator 1"),
    ((2, [0, 0b1, 0b1], 0b10), {}, "voice graph: modulators[2] = 0x1 beyond operator 1"),
    ((2, [0, 0b1], 0b10), dict(struct_size=40), "sots_voice_graph.struct_size 40 != 44"),
]


@pytest.mark.parametrize("graph,over,text", MALFORMED)
def test_every_malformed_graph_is_refused_with_its_own_text(hip, graph, over, text):
    lib = hip.load()
    g = hip.make_voice_graph(*graph)
    for k, v in over.items():
        setattr(g, k, v)
    cfg = hip.make_config(16, 16, hip.SYNTH_2OP, 10, None, [1.0] * 16)
    cfg.synth_kind, cfg.num_dimensions = hip.SYNTH_GRAPH, 2 * graph[0]
    h = C.c_void_p()
    assert lib.sots_create_graph(C.byref(cfg), C.byref(g), C.byref(h)) == -1 and not h.value
    assert lib.sots_last_error(None).decode() == text
    assert lib.sots_batch_create_graph(C.byref(cfg), C.byref(g), 2, C.byref(h)) == -1 and not h.value
    assert lib.sots_batch_last_error(None).decode() == text


def test_wrong_num_dimensions_and_null_arguments(hip):
    lib = hip.load()
    cfg, g = graph_cfg(hip, GRAPHS["chain3"], num_dimensions=4)
    h = C.c_void_p()
    assert lib.sots_create_graph(C.byref(cfg), C.byref(g), C.byref(h)) == -1
    assert lib.sots_last_error(None).decode() == "synth_kind 4 needs numDimensions 6, got 4"
    assert lib.sots_batch_create_graph(C.byref(cfg), C.byref(g), 2, C.byref(h)) == -1
    assert lib.sots_batch_last_error(None).decode() == "synth_kind 4 needs numDimensions 6, got 4"
    assert lib.sots_create_graph(C.byref(cfg), None, C.byref(h)) == -1
    assert lib.sots_last_error(None).decode() == "sots_create_graph: null argument"
    assert lib.sots_batch_create_graph(C.byref(cfg), None, 2, C.byref(h)) == -1
    assert lib.sots_batch_last_error(None).decode() == "sots_batch_create_graph: null argument"
    assert lib.sots_get_voice_graph(None, C.byref(g)) == -1
    assert lib.sots_last_error(None).decode() == "null context"


def test_a_good_graph_gets_as_far_as_the_device(hip):
    """without a GPU a valid graph configuration fails with SOTS_ERR_NO_DEVICE: nothing else is wrong with it"""
    lib = hip.load()
    for name in GRAPHS:
        cfg, g = graph_cfg(hip, GRAPHS[name])
        h = C.c_void_p()
        rc = lib.sots_create_graph(C.byref(cfg), C.byref(g), C.byref(h))
        if rc == 0:  # a GPU is present
            lib.sots_destroy(h)
        else:
            assert rc == -3 and not h.value, (name, lib.sots_last_error(None))
        rc = lib.sots_batch_create_graph(C.byref(cfg), C.byref(g), 2, C.byref(h))
        if rc == 0:
            lib.sots_batch_destroy(h)
        else:
            assert rc == -3 and not h.value, (name, lib.sots_batch_last_error(None))


# ---- sots_match: what parameters.json can get wrong about the voice, refused before any device work ----
from _graph_voice_match import CHAIN3, NO_DEVICE, run_match  # noqa: E402

JSON_REFUSALS = [
    ({"synth": "graph"}, 6, "type.HIP.synth \"graph\" needs type.HIP.voiceGraph"),
    ({"synth": "2op", "voiceGraph": CHAIN3}, 4, "type.HIP.voiceGraph needs type.HIP.synth \"graph\""),
    ({"synth": "graph", "voiceGraph": [0, 1]}, 6, "type.HIP.voiceGraph must be {\"operators\": n"),
    ({"synth": "graph", "voiceGraph": {"operators": 3, "modulators": [[], [0], [1]]}}, 6, "type.HIP.voiceGraph must be {\"operators\": n"),
    ({"synth": "graph", "voiceGraph": dict(CHAIN3, modulators=[[], [0]])}, 6, "modulators needs one list per operator (2 lists, 3 operators"),
    ({"synth": "graph", "voiceGraph": dict(CHAIN3, carriers=[2.5])}, 6, "operator indices are whole numbers"),
    ({"synth": "graph", "voiceGraph": dict(CHAIN3, modulators=[[], ["0"], [1]])}, 6, "operator indices are whole numbers"),
    ({"synth": "graph", "voiceGraph": CHAIN3}, 4, "evolutionary.numDimensions 4 must be 2 x type.HIP.voiceGraph.operators = 6"),
    ({"synth": "graph", "voiceGraph": CHAIN3, "renderMatch": True, "renderMode": "continuous"}, 6,
     "\"continuous\" and \"continuousGlide\" are not available with type.HIP.synth \"graph\""),
    # the topology itself: the library's rule, with its own text
    ({"synth": "graph", "voiceGraph": dict(CHAIN3, carriers=[])}, 6, "voice graph: no carrier"),
    ({"synth": "graph", "voiceGraph": dict(CHAIN3, carriers=[1, 2])}, 6, "voice graph: operator 1 is a carrier and modulates (one or the other)"),
    ({"synth": "graph", "voiceGraph": dict(CHAIN3, modulators=[[], [0], [0]])}, 6, "voice graph: operator 1 is dead: neither a carrier nor a modulator"),
    ({"synth": "graph", "voiceGraph": dict(CHAIN3, modulators=[[], [1], [1]])}, 6, "voice graph: modulators[1] = 0x2 has a bit at or above 1"),
    ({"synth": "graph", "voiceGraph": dict(CHAIN3, carriers=[2, 40])}, 6, "voice graph: carriers 0x80000004 has bits beyond operator 2"),
    ({"synth": "graph", "voiceGraph": {"operators": 1, "modulators": [[]], "carriers": [0]}}, 2, "voice graph: 1 operators outside 2..8"),
    ({"synth": "graph", "voiceGraph": CHAIN3, "numDevices": 2, "devices": [0, 0]}, 6, "sots_create_graph"),
]


@pytest.mark.parametrize("keys,dims,text", JSON_REFUSALS)
def test_sots_match_refuses_before_any_device_work(tmp_path, keys, dims, text):
    # no device is visible to this run: anything that reached the device first would fail with ITS text
    out, wav = run_match(tmp_path, "bad", keys, dims=dims, env=NO_DEVICE)
    assert out.returncode != 0
    assert text in out.stderr, out.stderr
    assert "no HIP device" not in out.stderr and not wav.exists()
