"""The per-operator feedback of the graph voice (sots_set_voice_feedback, include/sots_hip.h) in NumPy, beside
the model of the operator waveforms (tests/_graph_waveforms_model.py), from which everything else is taken: an operator
with an index beta_j other than 0 reads its shaped table at z = pos_j + (beta_j K) ((h1_j + h2_j) 0.5), wrapped once each way,
h1 and h2 its last two shaped values (before the level), both +0 at sample 0; pos_j itself is never touched.
graph_synth_feedback() is the model over all rows at once, graph_synth_feedback_scalar() restates it row by row in NumPy
float32 scalars with the definition's own if-statements."""
import numpy as np

from _graph_waveforms_model import (F32, GRAPHS, SAMPLE_RATE, SAW, SINE, SQUARE, W, edge_rows, graph_synth_waves, index_of,  # noqa: F401
                                    overflow_ranges, ranges, scale, shape_scalar, shape_table)

K = F32(32768 / (2 * np.pi))  # 0x45a2f983: the fp32 nearest W / 2 pi


def graph_synth_feedback(graph, waves, beta, values, pmin, pmax, n, table):
    """audio[rows][n] of values[rows][2 OPS] with operator j's waveform waves[j] and feedback index beta[j]"""
    ops, mods, carriers = graph
    assert len(waves) == ops and len(beta) == ops
    shaped = [shape_table(w, table) for w in waves]
    big = [F32(F32(b) * K) for b in beta]  # B_j: one fp32 product
    p = scale(np.atleast_2d(values), pmin, pmax)
    rows = p.shape[0]
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
                if beta[j] != 0:
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


def graph_synth_feedback_scalar(graph, waves, beta, values, pmin, pmax, n, table):
    """one row, NumPy float32 scalars, the definition's own if-statements"""
    ops, mods, carriers = graph
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
                if beta[j] != 0:
                    big = F32(F32(beta[j]) * K)
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
