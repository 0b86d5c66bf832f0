"""CPU-side checks of feedback indices as genes (sots_create_graph_genes): the NumPy model
(tests/_graph_feedback_genes_model.py) in its vectorised form against its scalar restatement on edge rows; rows of a constant
effective index against the model of the fixed setting (tests/_graph_feedback_model.py) bit for bit; the clamp; the rules
under ASan + UBSan in a stand-alone program (tests/graph_feedback_genes_san.cpp; nothing is loaded into Python under a
sanitizer); every refusal that needs no device through the C-ABI with its text; the symbols; and what sots_match refuses
before any device work.

The refusals of a LIVE handle (a fixed index on a gene operator, both continuous renderers, the getter on a fixed voice)
need a context and so a device: their rules and texts are held here through the stand-alone program, and through the C-ABI
in tests/test_gpu_graph_feedback_genes.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _graph_feedback_genes_model import (EDGE_VALUES, GRAPHS, K, dims, edge_gene_rows, edge_rows, effective_beta, effective_beta_scalar, gene_operators,
                                         gene_ranges, graph_synth_feedback, graph_synth_genes, graph_synth_genes_scalar, with_beta)
from _graph_voice_match import CHAIN3, NO_DEVICE, PMAX3, run_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sots_create_graph_genes", "sots_batch_create_graph_genes", "sots_get_voice_feedback_genes", "sots_batch_get_voice_feedback_genes"]
# (graph, mask): a carrier's gene, five genes, two carriers' genes
VOICES = [("2op", 0b10), ("stacks5", 0b11111), ("one_mod_two_carriers", 0b110)]


@pytest.fixture(scope="module")
def table(O):
    return O.wavetable()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """bit for bit, a NaN matching any NaN"""
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def codes(ops, rotation):
    return [(j + rotation) % 8 for j in range(ops)]


# ---- the layout and the effective index ----
def test_layout_and_effective_index():
    assert dims(2, 0b10) == 5 and dims(2, 0b11) == 6 and dims(5, 0b11111) == 15 and dims(8, 0) == 16
    assert gene_operators(5, 0b10100) == [2, 4]
    p = np.array([0.25, 1.0, 2.0, 2.5, np.inf, 0.0, -0.0, -1.0, -np.inf, np.nan, 2.0 ** -149], np.float32)
    want = np.array([0.25, 1.0, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0 ** -149], np.float32)
    got = effective_beta(p)
    assert np.array_equal(bits(got), bits(want))  # (bits: +0 for -0, for NaN and for every negative value)
    assert np.array_equal(bits(np.array([effective_beta_scalar(x) for x in p], np.float32)), bits(want))


# ---- vectorised against scalar, on edge rows ----
@pytest.mark.parametrize("name,mask,beta", [("2op", 0b10, [0.0, 0.0]), ("2op", 0b11, [0.0, 0.0]), ("chain3", 0b010, [0.5, 0.0, 0.0]),
                                            ("stacks5", 0b11111, [0.0] * 5)])
def test_edge_rows_vectorised_equal_scalar(table, name, mask, beta):
    """v = -0.5, 1.5, NaN, +inf and -inf in the beta genes and in the other genes, a row per (column, value); the genes'
    range [0.25, 1.75] sends -0.5 below 0 and 1.5 above 2"""
    g = GRAPHS[name]
    ops, d = g[0], dims(g[0], mask)
    pmin, pmax = gene_ranges(ops, mask, lo=0.25, hi=1.75)
    v = edge_gene_rows(d, 300 + d)
    assert v.shape[0] == 5 * d + 2 and len(EDGE_VALUES) == 5
    for col in range(d):
        column = v[2:, col]
        assert np.isnan(column).any() and np.isposinf(column).any() and np.isneginf(column).any() and (column == -0.5).any() and (column == 1.5).any()
    waves = codes(ops, 5)
    got = graph_synth_genes(g, waves, beta, mask, v, pmin, pmax, 64, table)
    for r in range(v.shape[0]):
        want = graph_synth_genes_scalar(g, waves, beta, mask, v[r], pmin, pmax, 64, table)
        assert same(got[r], want), (name, mask, r, v[r])


# ---- the anchor: a constant effective index is the fixed setting ----
@pytest.mark.parametrize("index", [0.25, 1.0, 2.0])
@pytest.mark.parametrize("name,mask", VOICES)
def test_constant_rows_equal_the_fixed_setting(table, name, mask, index):
    g = GRAPHS[name]
    ops = g[0]
    pmin, pmax = gene_ranges(ops, mask)
    plain = edge_rows(2 * ops, 6, 310 + ops)
    for waves in ([0] * ops, codes(ops, 6)):
        want = graph_synth_feedback(g, waves, [index if mask >> j & 1 else 0.0 for j in range(ops)], plain, pmin[:2 * ops], pmax[:2 * ops], 256, table)
        got = graph_synth_genes(g, waves, [0.0] * ops, mask, with_beta(plain, ops, mask, index), pmin, pmax, 256, table)
        assert np.array_equal(bits(got), bits(want)), (name, index, waves)
        row = graph_synth_genes_scalar(g, waves, [0.0] * ops, mask, with_beta(plain, ops, mask, index)[3], pmin, pmax, 256, table)
        assert np.array_equal(bits(row), bits(want[3]))
    assert not np.array_equal(bits(want), bits(graph_synth_feedback(g, waves, [0.0] * ops, plain, pmin[:2 * ops], pmax[:2 * ops], 256, table)))


# ---- the clamp ----
@pytest.mark.parametrize("name,mask", VOICES)
def test_values_outside_the_range_act_as_the_bounds(table, name, mask):
    """beta <= 0 and NaN act as +0 WITH THE CHAIN RUNNING, beta > 2 acts as 2.  The genes' range is [0, 2]: v = -0.5, -0.0,
    NaN and -inf give +0; v = 1.5 and +inf give 2"""
    g = GRAPHS[name]
    ops = g[0]
    pmin, pmax = gene_ranges(ops, mask)
    plain = edge_rows(2 * ops, 6, 320 + ops)
    waves = codes(ops, 6)

    def audio(gene_value):
        v = np.concatenate([plain, np.full((6, dims(ops, mask) - 2 * ops), gene_value, np.float32)], axis=1)
        return graph_synth_genes(g, waves, [0.0] * ops, mask, v, pmin, pmax, 256, table)

    zero, two = audio(0.0), audio(1.0)
    for x in (-0.5, -0.0, float("nan"), float("-inf")):
        assert np.array_equal(bits(audio(x)), bits(zero)), x
    for x in (1.5, float("inf"), 1.0000001):
        assert np.array_equal(bits(audio(x)), bits(two)), x
    assert np.array_equal(bits(two), bits(graph_synth_feedback(g, waves, [2.0 if mask >> j & 1 else 0.0 for j in range(ops)], plain,
                                                                pmin[:2 * ops], pmax[:2 * ops], 256, table)))
    assert not np.array_equal(bits(zero), bits(two))


def test_an_index_of_zero_runs_the_chain():
    """with pos in [0, W) the index of z = pos + (+0) g is that of pos; outside it the wraps of z are applied, where a
    skipped operator reads the clamp's entry.  An unmodulated operator of negative frequency shows the difference"""
    table = np.sin(np.arange(32768) / 32767.0 * 2 * np.pi).astype(np.float32)
    g = GRAPHS["additive"]  # two unmodulated carriers: no lower wrap of pos
    pmin, pmax = [-880.0, 0.0, 0.0, 0.0, 0.0], [0.0, 1.0, 440.0, 1.0, 2.0]
    v = np.array([[0.0, 1.0, 1.0, 0.0, 0.0]], np.float32)  # operator 0 at -880 Hz, level 1; its beta gene 0
    running = graph_synth_genes(g, [0, 0], [0.0, 0.0], 0b01, v, pmin, pmax, 64, table)
    skipped = graph_synth_feedback(g, [0, 0], [0.0, 0.0], v[:, :4], pmin[:4], pmax[:4], 64, table)
    assert not skipped[0, 1:].any(), "a negative phase is clamped to entry 0"
    assert np.abs(running[0, 1:]).max() > 0.01, "z is wrapped into the table"
    assert np.array_equal(bits(running[0]), bits(graph_synth_genes_scalar(g, [0, 0], [0.0, 0.0], 0b01, v[0], pmin, pmax, 64, table)))
    # positive frequencies: pos stays in [0, W) and the two agree bit for bit
    v[0, 0] = 1.0
    pmin[0], pmax[0] = 0.0, 880.0
    assert np.array_equal(bits(graph_synth_genes(g, [0, 0], [0.0, 0.0], 0b01, v, pmin, pmax, 64, table)),
                          bits(graph_synth_feedback(g, [0, 0], [0.0, 0.0], v[:, :4], pmin[:4], pmax[:4], 64, table)))


# ---- the rules, stand-alone, under the sanitizers ----
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_rules_are_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "graph_feedback_genes_san"
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", *SAN, "-o", str(exe),
                           os.path.join(ROOT, "tests", "graph_feedback_genes_san.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert "graph feedback genes: 52 checks, 0 failures" in out.stdout, out.stdout


# ---- the C-ABI without a device ----
def test_new_symbols_are_exported_and_declared(hip, pkg):
    lib = hip.load()
    header = open(os.path.join(ROOT, "include", "sots_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NEW:
        assert n in hip.EXPORTS and hasattr(lib, n), n
        assert re.search(r"\bint\s+%s\s*\(" % n, code), n
    assert not any(n.startswith("sots_group") and "genes" in n for n in hip.EXPORTS)  # islands do not take the voice
    for cls in (pkg.HipES, pkg.HipBatch):
        assert callable(cls.voice_feedback_genes)
    assert C.sizeof(hip.VoiceGraph) == 44
    assert "ALWAYS runs the feedback step" in header and "the index is that of pos_j" in header


def test_null_arguments_are_refused(hip):
    lib = hip.load()
    mask = C.c_uint32(7)
    assert lib.sots_get_voice_feedback_genes(None, C.byref(mask)) == -1
    assert lib.sots_last_error(None).decode() == "null context"
    assert lib.sots_batch_get_voice_feedback_genes(None, C.byref(mask)) == -1
    assert lib.sots_batch_last_error(None).decode() == "null batch"
    h = C.c_void_p()
    cfg = hip.make_config(32, 32, hip.SYNTH_GRAPH, 8, None, [1.0] * 5, graph=hip.make_voice_graph(*GRAPHS["2op"]), feedback_genes=0b10)
    assert lib.sots_create_graph_genes(C.byref(cfg), None, 0b10, C.byref(h)) == -1
    assert lib.sots_last_error(None).decode() == "sots_create_graph_genes: null argument"
    assert lib.sots_batch_create_graph_genes(C.byref(cfg), None, 0b10, 2, C.byref(h)) == -1
    assert lib.sots_batch_last_error(None).decode() == "sots_batch_create_graph_genes: null argument"
    assert mask.value == 7 and not h.value


def create_both(hip, name, mask, dims_, pmin, pmax, kind=None):
    """(code, text) of sots_create_graph_genes and of sots_batch_create_graph_genes for one configuration"""
    lib = hip.load()
    graph = hip.make_voice_graph(*GRAPHS[name])
    cfg = hip.make_config(32, 32, hip.SYNTH_GRAPH if kind is None else kind, 8, pmin, pmax, workgroup_size=32, graph=graph)
    cfg.num_dimensions = dims_
    h = C.c_void_p()
    rc = lib.sots_create_graph_genes(C.byref(cfg), C.byref(graph), mask, C.byref(h))
    one = (rc, lib.sots_last_error(None).decode())
    assert not h.value
    rc = lib.sots_batch_create_graph_genes(C.byref(cfg), C.byref(graph), mask, 2, C.byref(h))
    two = (rc, lib.sots_batch_last_error(None).decode())
    assert not h.value
    return one, two


PMAX2 = [3520.0, 8.0, 3520.0, 1.0]
CREATE_REFUSALS = [
    ("2op", 0b100, 5, None, PMAX2 + [2.0], "voice feedback genes: mask 0x4 has bits beyond operator 1"),
    ("dense8", 0x100, 16, None, [1.0] * 16, "voice feedback genes: mask 0x100 has bits beyond operator 7"),
    ("dense8", 0b1, 16, None, [1.0] * 16, "voice feedback genes: 8 operators and 1 feedback genes are 17 genes, more than 16"),
    ("seven", 0b111, 16, None, [1.0] * 16, "voice feedback genes: 7 operators and 3 feedback genes are 17 genes, more than 16"),
    ("2op", 0b10, 4, None, PMAX2 + [2.0], "voice feedback genes: 2 operators and 1 feedback genes need numDimensions 5, got 4"),
    ("2op", 0b10, 6, None, PMAX2 + [2.0], "voice feedback genes: 2 operators and 1 feedback genes need numDimensions 5, got 6"),
    ("2op", 0b10, 5, None, PMAX2 + [2.5], "voice feedback genes: gene 4 (operator 1's index) has the range 0..2.5, not 0 <= min <= max <= 2"),
    ("2op", 0b10, 5, [0.0] * 4 + [-0.5], PMAX2 + [1.0],
     "voice feedback genes: gene 4 (operator 1's index) has the range -0.5..1, not 0 <= min <= max <= 2"),
    ("2op", 0b10, 5, [0.0] * 4 + [1.5], PMAX2 + [1.0],
     "voice feedback genes: gene 4 (operator 1's index) has the range 1.5..1, not 0 <= min <= max <= 2"),
    ("2op", 0b11, 6, None, PMAX2 + [2.0, float("inf")],
     "voice feedback genes: gene 5 (operator 1's index) has the range 0..inf, not 0 <= min <= max <= 2"),
    ("stacks5", 0b10100, 12, None, [1.0] * 11 + [3.0],
     "voice feedback genes: gene 11 (operator 4's index) has the range 0..3, not 0 <= min <= max <= 2"),
]


@pytest.mark.parametrize("name,mask,dims_,pmin,pmax,text", CREATE_REFUSALS)
def test_create_refuses_before_any_device_work(hip, name, mask, dims_, pmin, pmax, text):
    """(this machine may have no device: anything that reached it first would fail with ITS text)"""
    for rc, got in create_both(hip, name, mask, dims_, pmin, pmax):
        assert rc == -1 and got == text, got


def test_a_nan_bound_and_a_fixed_voice_are_refused(hip):
    for rc, got in create_both(hip, "2op", 0b10, 5, None, PMAX2 + [float("nan")]):
        assert rc == -1 and got.startswith("voice feedback genes: gene 4 (operator 1's index) has the range 0.."), got
    # a fixed-voice configuration with a graph and a mask: the older rule speaks
    for rc, got in create_both(hip, "2op", 0b10, 4, None, PMAX2, kind=hip.SYNTH_2OP):
        assert rc == -1 and got == "a voice graph needs synth_kind 4 (SOTS_SYNTH_GRAPH), got 0", got


def test_mask_zero_is_sots_create_graph(hip):
    """the old rule with the old text; and a good configuration ends the same way through both entry points: a handle
    where there is a device, SOTS_ERR_NO_DEVICE (-3) with the same text where there is none - never a refusal of the
    configuration"""
    for rc, got in create_both(hip, "2op", 0, 5, None, PMAX2 + [2.0]):
        assert rc == -1 and got == "synth_kind 4 needs numDimensions 4, got 5", got
    lib = hip.load()
    graph = hip.make_voice_graph(*GRAPHS["2op"])
    cfg = hip.make_config(32, 32, hip.SYNTH_GRAPH, 8, None, PMAX2 + [2.0], graph=graph)
    assert cfg.num_dimensions == 4
    ends = []
    for create in (lambda h: lib.sots_create_graph(C.byref(cfg), C.byref(graph), C.byref(h)),
                   lambda h: lib.sots_create_graph_genes(C.byref(cfg), C.byref(graph), 0, C.byref(h))):
        h = C.c_void_p()
        rc = create(h)
        text = lib.sots_last_error(None).decode() if rc else ""
        assert (rc == 0 and h.value) or (rc == -3 and not h.value and text.startswith("no HIP device")), (rc, text)
        if h.value:
            mask = C.c_uint32(7)
            assert lib.sots_get_voice_feedback_genes(h, C.byref(mask)) == 0 and mask.value == 0
            lib.sots_destroy(h)
        ends.append((rc, text))
    assert ends[0] == ends[1], ends
    h = C.c_void_p()
    cfg.num_dimensions = 5  # sots_create_graph keeps its rule: a row of 5 genes is for the new entry point only
    assert lib.sots_create_graph(C.byref(cfg), C.byref(graph), C.byref(h)) == -1
    assert lib.sots_last_error(None).decode() == "synth_kind 4 needs numDimensions 4, got 5"


def test_python_refuses_a_mask_without_a_graph(hip, pkg):
    """a fixed voice has no feedback genes: the mask is not dropped silently"""
    for make in (lambda: pkg.HipES(32, 32, synth_kind=hip.SYNTH_2OP, audio_log2=8, param_max=PMAX2, feedback_genes=0b10),
                 lambda: pkg.HipBatch(2, 32, 32, synth_kind=hip.SYNTH_2OP, audio_log2=8, param_max=PMAX2, feedback_genes=[1]),
                 lambda: hip.make_config(32, 32, hip.SYNTH_2OP, 8, None, PMAX2, feedback_genes=0b10)):
        with pytest.raises(ValueError, match="feedback_genes needs SYNTH_GRAPH and graph="):
            make()


def test_python_layout(hip):
    graph = hip.make_voice_graph(*GRAPHS["stacks5"])
    assert hip.synth_dims(hip.SYNTH_GRAPH, graph) == 10
    assert hip.synth_dims(hip.SYNTH_GRAPH, graph, 0b11111) == 15 and hip.synth_dims(hip.SYNTH_GRAPH, graph, [1, 3]) == 12
    cfg = hip.make_config(32, 32, hip.SYNTH_GRAPH, 8, None, [1.0] * 15, graph=graph, feedback_genes=[0, 1, 2, 3, 4])
    assert cfg.num_dimensions == 15 and cfg.param_max[14] == 1.0 and cfg.param_max[15] == 0.0


# ---- sots_match: what parameters.json can get wrong about the key, refused before any device work ----
GRAPH = {"synth": "graph", "voiceGraph": CHAIN3}
PMAX_G = PMAX3 + [2.0]
JSON_REFUSALS = [
    ({"synth": "2op", "voiceFeedbackGenes": [0, 1]}, 4, PMAX3[:4], "type.HIP.voiceFeedbackGenes needs type.HIP.synth \"graph\""),
    ({"voiceFeedbackGenes": [0, 1]}, 4, PMAX3[:4], "type.HIP.voiceFeedbackGenes needs type.HIP.synth \"graph\""),
    (dict(GRAPH, voiceFeedbackGenes=[0, 1]), 7, PMAX_G, "type.HIP.voiceFeedbackGenes needs one 0 or 1 per operator (2 entries, 3 operators)"),
    (dict(GRAPH, voiceFeedbackGenes=[0, 1, 0, 0]), 7, PMAX_G, "type.HIP.voiceFeedbackGenes needs one 0 or 1 per operator (4 entries, 3 operators)"),
    (dict(GRAPH, voiceFeedbackGenes=1), 7, PMAX_G, "type.HIP.voiceFeedbackGenes needs one 0 or 1 per operator (not a list, 3 operators)"),
    (dict(GRAPH, voiceFeedbackGenes=[0, 2, 0]), 7, PMAX_G, "type.HIP.voiceFeedbackGenes: an entry that is neither 0 nor 1"),
    (dict(GRAPH, voiceFeedbackGenes=[0, 1, 0], voiceFeedback=[0, 0.5, 0]), 7, PMAX_G,
     "type.HIP.voiceFeedbackGenes: operator 1 also has a type.HIP.voiceFeedback of 0.500000 (one or the other)"),
    (dict(GRAPH, voiceFeedbackGenes=[0, 1, 0]), 6, PMAX3,
     "type.HIP.voiceFeedbackGenes: 3 operators and 1 feedback genes need numDimensions 7 with 7 paramMins and paramMaxs, got 6, 6 and 6"),
    (dict(GRAPH, voiceFeedbackGenes=[0, 1, 0]), 7, PMAX3,
     "type.HIP.voiceFeedbackGenes: 3 operators and 1 feedback genes need numDimensions 7 with 7 paramMins and paramMaxs, got 7, 6 and 6"),
    (dict(GRAPH, voiceFeedbackGenes=[0, 1, 0], renderMode="graphContinuous"), 7, PMAX_G,
     "type.HIP.voiceFeedbackGenes: every row has its own feedback index, which type.HIP.renderMode \"graphContinuous\" cannot render"),
    (dict(GRAPH, voiceFeedbackGenes=[0, 1, 0], renderMode="graphFeedback"), 7, PMAX_G,
     "type.HIP.voiceFeedbackGenes: every row has its own feedback index, which type.HIP.renderMode \"graphFeedback\" cannot render"),
    (dict(GRAPH, voiceFeedbackGenes=[0, 1, 0], renderMode="graphContinuousGlide"), 7, PMAX_G,
     "type.HIP.voiceFeedbackGenes: every row has its own feedback index, which type.HIP.renderMode \"graphContinuousGlide\" cannot render"),
    (dict(GRAPH, voiceFeedbackGenes=[0, 1, 0], renderMode="graphFeedbackGlide"), 7, PMAX_G,
     "type.HIP.voiceFeedbackGenes: every row has its own feedback index, which type.HIP.renderMode \"graphFeedbackGlide\" cannot render"),
]
DENSE8 = {"operators": 8, "modulators": [[]] + [list(range(min(j, 6))) for j in range(1, 8)], "carriers": [6, 7]}


@pytest.mark.parametrize("keys,dims_,pmax,text", JSON_REFUSALS)
def test_sots_match_refuses_before_any_device_work(tmp_path, keys, dims_, pmax, text):
    # no device is visible to this run: anything that reached the device first would fail with ITS text
    out, wav = run_match(tmp_path, "bad", keys, dims=dims_, pmax=pmax, env=NO_DEVICE)
    assert out.returncode != 0
    assert text in out.stderr, out.stderr
    assert "no HIP device" not in out.stderr and not wav.exists()


def test_sots_match_refuses_more_than_sixteen_genes(tmp_path):
    keys = {"synth": "graph", "voiceGraph": DENSE8, "voiceFeedbackGenes": [1, 0, 0, 0, 0, 0, 0, 0]}
    out, wav = run_match(tmp_path, "wide", keys, dims=17, pmax=[1.0] * 17, env=NO_DEVICE)
    assert out.returncode != 0
    assert "type.HIP.voiceFeedbackGenes: 8 operators and 1 feedback genes are 17 genes, more than 16" in out.stderr, out.stderr
    assert "no HIP device" not in out.stderr and not wav.exists()


def test_sots_match_takes_a_good_key_as_far_as_the_device(tmp_path):
    out, wav = run_match(tmp_path, "good", dict(GRAPH, voiceFeedbackGenes=[0, 1, 0], voiceFeedback=[1.0, 0, 0]), dims=7, pmax=PMAX_G, env=NO_DEVICE)
    assert out.returncode != 0 and "no HIP device" in out.stderr and "voiceFeedbackGenes" not in out.stderr
