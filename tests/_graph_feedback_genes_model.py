"""Feedback indices as genes (sots_create_graph_genes, include/sots_hip.h) in NumPy, beside the model of the
fixed feedback setting (tests/_graph_feedback_model.py), from which everything else is taken.  A row has 2 OPS + E genes;
gene 2 OPS + r is the feedback index of the operator with the r-th set bit of the mask.  Scaled like every gene, then

    beta = p > 0 ? fminf(p, 2) : +0,    B = beta K

and a gene operator ALWAYS runs the feedback step with its row's B (h1, h2, both wraps of z), also where beta is +0.  The
other operators keep the fixed setting's rule: an index other than 0 runs the step, 0 skips it.
graph_synth_genes() is the model over all rows at once, graph_synth_genes_scalar() restates it row by row in NumPy float32
scalars with the definition's own if-statements."""
import numpy as np

from _graph_feedback_model import (F32, GRAPHS, K, SAMPLE_RATE, W, edge_rows, graph_synth_feedback, index_of, ranges, scale,  # noqa: F401
                                   shape_scalar, shape_table)

BETA_MAX = F32(2.0)


def gene_operators(ops, mask):
    """the operators whose index is a gene, ascending: operator gene_operators[r] reads column 2 OPS + r"""
    return [j for j in range(ops) if mask >> j & 1]


def dims(ops, mask):
    return 2 * ops + len(gene_operators(ops, mask))


def effective_beta(p):
    """beta of scaled genes p (any shape): NaN, negatives and zeros give +0, values above 2 give 2"""
    p = np.asarray(p, F32)
    with np.errstate(invalid="ignore"):
        return np.where(p > F32(0), np.minimum(p, BETA_MAX), F32(0)).astype(F32)


def effective_beta_scalar(p):
    p = F32(p)
    if p > F32(0):  # (false for NaN)
        return BETA_MAX if p > BETA_MAX else p
    return F32(0)


def gene_ranges(ops, mask, lo=0.0, hi=2.0, **kw):
    """ranges(ops) of tests/_graph_voice_model.py with [lo, hi] for every feedback gene behind them"""
    pmin, pmax = ranges(ops, **kw)
    e = len(gene_operators(ops, mask))
    return pmin + [lo] * e, pmax + [hi] * e


def with_beta(values, ops, mask, beta, lo=0.0, hi=2.0):
    """values[rows][2 OPS] with the gene columns behind them, set so that every gene scales to exactly `beta` (a number or
    one per gene operator) in the range [lo, hi]: v = (beta - lo) / (hi - lo) must be exact in fp32, and is checked"""
    v = np.atleast_2d(np.asarray(values, F32))
    genes = gene_operators(ops, mask)
    b = np.broadcast_to(np.asarray(beta, F32), (len(genes),))
    col = ((b - F32(lo)) / (F32(hi) - F32(lo))).astype(F32)
    assert np.array_equal((F32(lo) + col * (F32(hi) - F32(lo))).astype(F32), b), "the gene does not scale to beta exactly"
    return np.concatenate([v, np.broadcast_to(col, (v.shape[0], len(genes)))], axis=1).astype(F32)


def graph_synth_genes(graph, waves, beta, mask, values, pmin, pmax, n, table):
    """audio[rows][n] of values[rows][2 OPS + E]; beta[j]: the fixed index of an operator outside the mask (0 inside it)"""
    ops, mods, carriers = graph
    genes = gene_operators(ops, mask)
    assert len(waves) == ops and len(beta) == ops and all(beta[j] == 0 for j in genes)
    shaped = [shape_table(w, table) for w in waves]
    p = scale(np.atleast_2d(values), pmin, pmax)
    rows = p.shape[0]
    assert p.shape[1] == 2 * ops + len(genes)
    big = [np.full(rows, F32(F32(b) * K), F32) for b in beta]  # B_j: one fp32 product
    for r, j in enumerate(genes):
        big[j] = (effective_beta(p[:, 2 * ops + r]) * K).astype(F32)
    c = F32(W) / F32(SAMPLE_RATE)
    wf = F32(W)
    half = F32(0.5)
    f = [p[:, 2 * j] for j in range(ops)]
    a = [p[:, 2 * j + 1] for j in range(ops)]
    with np.errstate(over="ignore"):
        amp = [a[j] if carriers >> j & 1 else f[j] * a[j] for j in range(ops)]
    pos = [np.zeros(rows, F32) for _ in range(ops)]
    h1 = [np.zeros(rows, F32) for _ in range(ops)]
    h2 = [np.zeros(rows, F32) for _ in range(ops)]
    count = bin(carriers).count("1")
    audio = np.zeros((rows, n), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(n):
            o = [None] * ops
            for j in range(ops):
                if j in genes or beta[j] != 0:  # (a gene operator: always, whatever its rows' beta)
                    g = ((h1[j] + h2[j]).astype(F32) * half).astype(F32)
                    z = (pos[j] + (big[j] * g).astype(F32)).astype(F32)
                    z = np.where(z >= wf, z - wf, z).astype(F32)
                    z = np.where(z < F32(0), z + wf, z).astype(F32)
                    t = shaped[j][index_of(z)]
                    h2[j], h1[j] = h1[j], t
                else:  # skipped, not computed with an offset of 0
                    t = shaped[j][index_of(pos[j])]
                o[j] = t * amp[j]
                cur = None
                for k in range(j):
                    if mods[j] >> k & 1:
                        cur = o[k] if cur is None else cur + o[k]
                cur = f[j] if cur is None else cur + f[j]
                q = pos[j] + c * cur
                q = np.where(q >= wf, q - wf, q)
                if mods[j]:
                    q = np.where(q < F32(0), q + wf, q)
                pos[j] = q.astype(F32)
            y = None
            for j in range(ops):
                if carriers >> j & 1:
                    y = o[j] if y is None else y + o[j]
            audio[:, s] = y / F32(count) if count > 1 else y
    return audio


def graph_synth_genes_scalar(graph, waves, beta, mask, values, pmin, pmax, n, table):
    """one row, NumPy float32 scalars, the definition's own if-statements"""
    ops, mods, carriers = graph
    genes = gene_operators(ops, mask)
    p = scale(values, pmin, pmax)
    c = F32(W) / F32(SAMPLE_RATE)
    wf = F32(W)
    with np.errstate(over="ignore"):
        amp = [p[2 * j + 1] if carriers >> j & 1 else p[2 * j] * p[2 * j + 1] for j in range(ops)]
    pos = [F32(0)] * ops
    h1 = [F32(0)] * ops
    h2 = [F32(0)] * ops
    count = bin(carriers).count("1")
    out = np.zeros(n, F32)

    def at(x):
        if x >= wf:
            return W - 1
        if not x > F32(0):
            return 0
        return int(x)

    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(n):
            o = [F32(0)] * ops
            for j in range(ops):
                gene = mask >> j & 1
                if gene or beta[j] != 0:
                    if gene:
                        b = effective_beta_scalar(p[2 * ops + genes.index(j)])
                    else:
                        b = F32(beta[j])
                    big = F32(b * K)
                    g = F32(F32(h1[j] + h2[j]) * F32(0.5))
                    z = F32(pos[j] + F32(big * g))
                    if z >= wf:
                        z = F32(z - wf)
                    if z < F32(0):
                        z = F32(z + wf)
                    t = shape_scalar(waves[j], at(z), table)
                    h2[j] = h1[j]
                    h1[j] = t
                else:
                    t = shape_scalar(waves[j], at(pos[j]), table)
                o[j] = F32(t * amp[j])
                ins = [o[i] for i in range(j) if mods[j] >> i & 1]
                if ins:
                    cur = ins[0]
                    for x in ins[1:]:
                        cur = F32(cur + x)
                    cur = F32(cur + p[2 * j])
                else:
                    cur = p[2 * j]
                q = F32(pos[j] + F32(c * cur))
                if q >= wf:
                    q = F32(q - wf)
                if mods[j] and q < F32(0):
                    q = F32(q + wf)
                pos[j] = q
            heard = [o[j] for j in range(ops) if carriers >> j & 1]
            y = heard[0]
            for x in heard[1:]:
                y = F32(y + x)
            out[s] = F32(y / F32(count)) if count > 1 else y
    return out


EDGE_VALUES = [-0.5, 1.5, float("nan"), float("inf"), float("-inf")]


def edge_gene_rows(d, seed, rows=None):
    """rows of edge_rows() with v = -0.5, 1.5, NaN, +inf and -inf in one column each: a row per (column, value), so the
    feedback genes and the other genes are each hit by every value; rows 2 .. 5 d + 1 are those, the rest are random"""
    specials = EDGE_VALUES
    count = d * len(specials) + 2
    v = edge_rows(d, count if rows is None else rows, seed)
    assert v.shape[0] >= count
    k = 2
    for col in range(d):
        for x in specials:
            v[k, col] = x
            k += 1
    return v
