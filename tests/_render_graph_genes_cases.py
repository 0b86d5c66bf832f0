"""The contexts, rows and shapes that tests/test_render_graph_genes_cpu.py (on the model) and tests/test_gpu_render_graph_genes.py
(on the device) render, so that what the CPU file asserts of the cases holds for what the GPU file runs."""
import numpy as np

import _graph_feedback_genes_model as GG
import _render_graph_continuous_model as GM

GRAPHS = GM.GRAPHS
N = 256
F = np.float32

# (graph, waveform codes or None, fixed indices, mask): the carrier's index a gene (D = 5); a gene operator beside one of a fixed
# index and one without feedback (D = 7); five gene operators, D = 15, the voice of tests/test_gpu_graph_feedback_genes.py
CASES = {"2op_carrier": ("2op", None, [0.0, 0.0], 0b10),
         "chain3_gene_beside_fixed": ("chain3", None, [0.75, 0.0, 0.0], 0b010),
         "stacks5_all": ("stacks5", [0, 7, 0, 1, 6], [0.0] * 5, 0b11111)}


def waveform_case(w):
    """code w on a gene modulator (operator 0) and on the gene carrier (operator 2) of chain3: D = 8"""
    return ("chain3", [w, 0, w], [0.0, 0.0, 0.0], 0b101)


# (rows, hop): 862 samples, one device tile per operator; 7225 samples, across a 4096 scan tile and eight chain tiles; a row per
# sample; rows that do not overlap
SHAPES = {"7x101": (7, 101), "70x101": (70, 101), "7x1": (7, 1), "7xN": (7, N)}

# What a feedback gene holds.  Under the range [0, 2]: +0, +0 (below the range), 2, between, 2 (above the range), +0 (NaN),
# 2 (+inf), +0 (-inf): both bounds and every branch of effective_feedback
EDGE = [0.0, -0.5, 1.0, 0.37, 1.5, float("nan"), float("inf"), float("-inf")]
QUIET = [0.0, -0.5, float("nan"), float("-inf")]  # all +0
QUIET_ROWS = range(18, 33)  # of a 70-row track at hop 101: what samples 2048 .. 3071, a device tile, look at, HOLD or GLIDE


def dims(case):
    name, _, _, mask = case
    return GG.dims(GRAPHS[name][0], mask)


def ranges(case, lo=0.0, hi=2.0):
    """(pmin, pmax) of D entries: the GPU tests' ranges of the 2 OPS genes, [lo, hi] for every feedback gene"""
    name, _, _, mask = case
    return GG.gene_ranges(GRAPHS[name][0], mask, lo, hi)


def rows_of(case, rows=7):
    """values[rows][D]: the rows the tests of the fixed setting render (tests/_render_graph_continuous_model.py) with the gene
    columns behind them.  Column c holds EDGE from entry 3 c on in rows 0 .. 7, so that in column 0 rows 0 and 1 are quiet
    (effective index +0: the first 256 samples of a rendering settle at once); further rows are random in [0, 1), except
    QUIET_ROWS, which are quiet in every column"""
    name, _, _, mask = case
    ops = GRAPHS[name][0]
    e = len(GG.gene_operators(ops, mask))
    v = GM.graph_rows(ops, rows, 100 + ops)
    g = np.random.default_rng(7 + ops).random((rows, e), dtype=F)
    for c in range(e):
        for r in range(min(rows, len(EDGE))):
            g[r, c] = EDGE[(r + 3 * c) % len(EDGE)]
        for r in QUIET_ROWS:
            if r < rows:
                g[r, c] = QUIET[(r + c) % len(QUIET)]
    return np.concatenate([v, g], axis=1).astype(F)


def finite_rows(case, rows=7):
    """rows_of() with every gene finite: what anchor (b) takes (a range [b, b] scales any finite gene to b)"""
    v = rows_of(case, rows)
    ops = GRAPHS[case[0]][0]
    g = v[:, 2 * ops:]
    g[~np.isfinite(g)] = 0.61
    return v


def fixed_twin(case, b):
    """the case with the index b set on every gene operator: (fixed indices, the columns of a row that such a voice takes)"""
    name, _, beta, mask = case
    ops = GRAPHS[name][0]
    return [b if mask >> j & 1 else beta[j] for j in range(ops)], slice(0, 2 * ops)
