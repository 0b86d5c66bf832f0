"""What tests/test_gpu_render_graph_feedback.py renders, stated once so that tests/test_render_graph_feedback_cpu.py can assert on
the NumPy model what these cases cover.  A case is (graph name, waveform codes or None, feedback indices); the rows are
_render_graph_continuous_model.graph_rows(ops, rows, 100 + ops) under _graph_waveforms_model.ranges(ops), as in the tests of 4.16."""
from _render_graph_continuous_model import MIXED8

BASE_SHAPE = (256, 7, 101)  # N, rows, hop: S = 862 samples, no multiple of 4 - the pass's end cuts a quad

BASE = [
    ("2op", None, [0.0, 0.75]),  # the carrier: its t buffer is read by the mix
    ("2op", None, [0.75, 0.0]),  # the modulator: its t buffer is read by the next level
    ("chain3", None, [0.5, 1.0, 2.0]),
    ("additive", None, [1.0, 0.5]),  # two chains in one launch
    ("one_mod_two_carriers", None, [1.0, 0.0, 0.0]),
    ("dense8", MIXED8, [0.5, 0, 0, 1.0, 0, 0, 0, 1.5]),
]
BASE_IDS = ["2op-carrier", "2op-modulator", "chain3", "additive", "one_mod_two_carriers", "dense8-mixed"]


def waveform_case(w):
    """code w on a feedback modulator (operator 0) and on a feedback carrier (operator 2) of chain3"""
    return ("chain3", [w, 0, w], [1.0, 0.0, 0.75])


# several tiles with a carry: (graph, waves, beta, rows, N, hop) - 17 920 samples, 17.5 tiles of the relaxation, 4.4 of the scans
CHAIN3_CARRY = ("chain3", None, [0.5, 1.0, 2.0], 70, 256, 256)

# one kernel set with and without feedback (graph, N, hop, rows, samples per pass): 5312 samples, two passes of which the first
# is one full tile of the scans
SHARED = ("chain3", 256, 64, 80, 4096)


def mixed_level_cases():
    """dense8 with feedback on operator 2 only: operator 3 reads the flagged operator 2 beside the unflagged 0 and 1.  SQUARE
    on the flagged one and SINE on the others (the level reads the table for the unflagged ones), and the other way round (no
    level launch reads it; only operator 2's chain does)"""
    beta = [0.0, 0.0, 1.0] + [0.0] * 5
    return [("dense8", [0, 0, 6, 0, 0, 0, 0, 0], beta), ("dense8", [6, 6, 0, 6, 6, 6, 6, 6], beta)]
