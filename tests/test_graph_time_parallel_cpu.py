"""CPU-side checks of the graph voice's time-parallel synthesis form (sots_set_graph_synth_form,
sots_graph_time_parallel_capacity): capacity and levels of the thirteen graphs against a restatement of the
plan in Python, the refusals that need no device through the C-ABI and through sots_match, and the plan rule under
ASan + UBSan in a stand-alone program (tests/graph_time_parallel_san.cpp; nothing is loaded into Python under a sanitizer)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from _graph_voice_model import GRAPHS
from _graph_voice_match import CHAIN3, NO_DEVICE, run_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_BYTES, LDS_BYTES = (64 + 4) * 4, 31 * 1024


def plan(graph):
    """(capacity, levels, rows per individual): the schedule of DESIGN.md 4.20, restated.  An operator scans at tick[j] and
    makes its output a tick later; a reader scans two ticks after its latest modulator; the mixer - the last carrier - runs
    after every other carrier; then everybody moves as late as the readers allow.  An output is kept from the tick it is
    made to the tick it is last read: that many blocks of ring, and two blocks of phases per operator."""
    ops, mods, carriers = graph
    level = [0] * ops
    for j in range(ops):
        level[j] = max([level[i] + 1 for i in range(j) if mods[j] >> i & 1], default=0)
    tick = [2 * l for l in level]
    heard = [j for j in range(ops) if carriers >> j & 1]
    mixer = max(heard, key=lambda j: (tick[j], j))
    if any(tick[j] == tick[mixer] for j in heard if j != mixer):
        tick[mixer] += 1
    readers = lambda j: [tick[k] for k in range(j + 1, ops) if mods[k] >> j & 1]  # noqa: E731
    for j in reversed(range(ops)):
        if j != mixer:
            tick[j] = max(tick[j], min([t - 2 for t in readers(j)] + ([tick[mixer] - 1] if j in heard else [])))
    rows = 2 * ops
    for j in range(ops):
        if j != mixer:
            rows += max(readers(j) + ([tick[mixer] + 1] if j in heard else [])) - tick[j]
    return min(LDS_BYTES // (rows * ROW_BYTES), 64), max(level) + 1, rows


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_capacity_and_levels_equal_the_restated_plan(hip, name):
    cap, levels = hip.graph_time_parallel_capacity(hip.make_voice_graph(*GRAPHS[name]))
    want_cap, want_levels, rows = plan(GRAPHS[name])
    assert (cap, levels) == (want_cap, want_levels), (name, rows)
    assert cap * rows * ROW_BYTES <= LDS_BYTES  # no plan uses more than the 31 KiB beside the table
    if GRAPHS[name][0] <= 4:
        assert cap >= 8, name  # the shipped workload's share of a CU: 64 chunks x 32 rows over 256 CUs


def test_the_capacities_and_levels_the_design_names(hip):
    cap = {name: hip.graph_time_parallel_capacity(hip.make_voice_graph(*g)) for name, g in GRAPHS.items()}
    assert cap["2op"][0] >= 19  # k_synth_tp's
    assert (cap["chain8"][1], cap["additive8"][1], cap["triple"][1]) == (8, 1, 2)
    assert all(c >= 1 for c, _ in cap.values())


def test_new_symbols_and_codes(hip):
    lib = hip.load()
    for n in ("sots_set_graph_synth_form", "sots_get_graph_synth_form", "sots_batch_set_graph_synth_form",
              "sots_batch_get_graph_synth_form", "sots_graph_time_parallel_capacity"):
        assert n in hip.EXPORTS and hasattr(lib, n), n
    assert (hip.GRAPH_FORM_AUTO, hip.GRAPH_FORM_LANES, hip.GRAPH_FORM_TIME_PARALLEL) == (0, 1, 2)
    assert hip.GRAPH_FORM_NAMES == {"auto": 0, "lanes": 1, "timeParallel": 2}


def test_refusals_that_need_no_device(hip):
    lib = hip.load()
    cap, levels = C.c_uint32(77), C.c_uint32(77)
    assert lib.sots_graph_time_parallel_capacity(None, C.byref(cap), C.byref(levels)) == -1
    assert lib.sots_last_error(None).decode() == "voice graph: null pointer"
    g = hip.make_voice_graph(*GRAPHS["2op"])
    g.struct_size = 40
    assert lib.sots_graph_time_parallel_capacity(C.byref(g), C.byref(cap), C.byref(levels)) == -1
    assert lib.sots_last_error(None).decode() == "sots_voice_graph.struct_size 40 != 44"
    for graph, text in [((3, [0, 0b1, 0b1], 0b100), "voice graph: operator 1 is dead: neither a carrier nor a modulator"),
                        ((2, [0, 0b1], 0), "voice graph: no carrier"),
                        ((9, [0] * 8, 1), "voice graph: 9 operators outside 2..8")]:
        bad = hip.make_voice_graph(*graph)
        assert lib.sots_graph_time_parallel_capacity(C.byref(bad), C.byref(cap), C.byref(levels)) == -1
        assert lib.sots_last_error(None).decode() == text
    assert (cap.value, levels.value) == (77, 77)  # a refusal writes nothing
    # either output may be left out
    good = hip.make_voice_graph(*GRAPHS["chain3"])
    assert lib.sots_graph_time_parallel_capacity(C.byref(good), None, C.byref(levels)) == 0 and levels.value == 3
    assert lib.sots_graph_time_parallel_capacity(C.byref(good), C.byref(cap), None) == 0 and cap.value == plan(GRAPHS["chain3"])[0]
    # null handles
    req, eff = C.c_uint32(), C.c_uint32()
    assert lib.sots_set_graph_synth_form(None, 1) == -1 and lib.sots_last_error(None).decode() == "null context"
    assert lib.sots_get_graph_synth_form(None, C.byref(req), C.byref(eff)) == -1 and lib.sots_last_error(None).decode() == "null context"
    assert lib.sots_batch_set_graph_synth_form(None, 1) == -1 and lib.sots_batch_last_error(None).decode() == "null batch"
    assert lib.sots_batch_get_graph_synth_form(None, C.byref(req), C.byref(eff)) == -1 and lib.sots_batch_last_error(None).decode() == "null batch"


JSON_REFUSALS = [
    ({"synth": "2op", "graphSynthForm": "timeParallel"}, 4, "type.HIP.graphSynthForm needs type.HIP.synth \"graph\""),
    ({"synth": "graph", "voiceGraph": CHAIN3, "graphSynthForm": "fast"}, 6, "type.HIP.graphSynthForm must be \"auto\", \"lanes\" or \"timeParallel\""),
    ({"synth": "graph", "voiceGraph": CHAIN3, "graphSynthForm": 2}, 6, "type.HIP.graphSynthForm must be \"auto\", \"lanes\" or \"timeParallel\""),
]


@pytest.mark.parametrize("keys,dims,text", JSON_REFUSALS)
def test_sots_match_refuses_the_key_before_any_device_work(tmp_path, keys, dims, text):
    # no device is visible to this run: anything that reached the device first would fail with ITS text
    out, wav = run_match(tmp_path, "bad", keys, dims=dims, env=NO_DEVICE)
    assert out.returncode != 0
    assert text in out.stderr, out.stderr
    assert "no HIP device" not in out.stderr and not wav.exists()


# ---- the plan rule, stand-alone, under the sanitizers ----
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def test_the_plan_rule_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "graph_time_parallel_san"
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", *SAN, "-o", str(exe),
                           os.path.join(ROOT, "tests", "graph_time_parallel_san.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    m = re.search(r"graph time parallel: (\d+) legal graphs, (\d+) checks, 0 failures", out.stdout)
    assert m and int(m.group(1)) > 20 and int(m.group(2)) > 500, out.stdout
