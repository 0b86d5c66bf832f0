"""The operator waveforms of the graph voice (sots_set_voice_waveforms, include/sots_hip.h) in NumPy, beside the model of the
all-sine voice (tests/_graph_voice_model.py), from which everything but the shapes is taken: step 1 of the voice becomes
o_j = shape(w_j, i) A_j with i the index tab_at uses.  A shape is a function of the index alone, so shape_table(w, table) -
its 32768 values - is a table like any other: graph_synth_waves() reads operator j's value from table number w_j and is
graph_synth() otherwise, operation by operation.  graph_synth_waves_scalar() restates it row by row with the definition's
own if-statements on the index, without the derived tables."""
import numpy as np

from _graph_voice_model import F32, GRAPHS, SAMPLE_RATE, W, edge_rows, graph_synth, overflow_ranges, ranges, scale  # noqa: F401

SINE, HALF, ABS, PULSE, EVEN, ABS_EVEN, SQUARE, SAW = range(8)
WAVES = range(8)
NAMES = ["sine", "half", "abs", "pulse", "even", "absEven", "square", "saw"]


def shape_table(w, table):
    """shape(w, i) for i = 0 .. W-1: every case decided on the index, never on the sign of an entry"""
    t = np.asarray(table, F32)
    i = np.arange(W)
    zero = np.zeros(W, F32)  # +0.0f
    low = i < W // 2
    twice = t[(2 * i) % W]  # T[2i] where i < W/2; the rest is masked out below
    if w == SINE:
        return t.copy()
    if w == HALF:
        return np.where(low, t, zero)
    if w == ABS:
        return np.abs(t)
    if w == PULSE:
        return np.where((i & (W // 4)) == 0, np.abs(t), zero)
    if w == EVEN:
        return np.where(low, twice, zero)
    if w == ABS_EVEN:
        return np.where(low, np.abs(twice), zero)
    if w == SQUARE:
        return np.where(low, F32(1.0), F32(-1.0)).astype(F32)
    if w == SAW:
        return (i.astype(F32) * F32(2.0 ** -14) - F32(1.0)).astype(F32)
    raise ValueError(w)


def index_of(pos):
    """clamp((int)pos, 0, W-1), decided on the float: at or beyond W -> W-1, negative or NaN -> 0"""
    with np.errstate(invalid="ignore"):
        idx = np.where(pos >= F32(W), F32(W - 1), np.where(pos > F32(0), pos, F32(0)))
    return idx.astype(np.int64)


def graph_synth_waves(graph, waves, values, pmin, pmax, n, table, seen=None):
    """audio[rows][n] of values[rows][2 OPS] with operator j's waveform waves[j].  seen: a dict that is told which
    (code, index) pairs were read - seen[(w, "modulated" | "plain", "modulator" | "carrier")] is a set of index regions
    i // (W/8)"""
    ops, mods, carriers = graph
    assert len(waves) == ops
    shaped = [shape_table(w, table) for w in waves]
    p = scale(np.atleast_2d(values), pmin, pmax)
    rows = p.shape[0]
    c = F32(W) / F32(SAMPLE_RATE)
    wf = F32(W)
    f = [p[:, 2 * j] for j in range(ops)]
    a = [p[:, 2 * j + 1] for j in range(ops)]
    with np.errstate(over="ignore"):
        amp = [a[j] if carriers >> j & 1 else f[j] * a[j] for j in range(ops)]
    pos = [np.zeros(rows, F32) for _ in range(ops)]
    count = bin(carriers).count("1")
    audio = np.zeros((rows, n), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(n):
            o = [None] * ops
            for j in range(ops):
                i = index_of(pos[j])
                o[j] = shaped[j][i] * amp[j]
                if seen is not None:
                    key = (waves[j], "modulated" if mods[j] else "plain", "carrier" if carriers >> j & 1 else "modulator")
                    seen.setdefault(key, set()).update(np.unique(i // (W // 8)).tolist())
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


def shape_scalar(w, i, table):
    """the table of the definition, row by row"""
    t = table
    if w == SINE:
        return t[i]
    if w == HALF:
        return t[i] if i < W // 2 else F32(0.0)
    if w == ABS:
        return F32(abs(t[i]))
    if w == PULSE:
        return F32(abs(t[i])) if (i & (W // 4)) == 0 else F32(0.0)
    if w == EVEN:
        return t[2 * i] if i < W // 2 else F32(0.0)
    if w == ABS_EVEN:
        return F32(abs(t[2 * i])) if i < W // 2 else F32(0.0)
    if w == SQUARE:
        return F32(1.0) if i < W // 2 else F32(-1.0)
    if w == SAW:
        return F32(F32(F32(i) * F32(2.0 ** -14)) - F32(1.0))
    raise ValueError(w)


def graph_synth_waves_scalar(graph, waves, values, pmin, pmax, n, table):
    """one row, NumPy float32 scalars, the definition's own if-statements"""
    ops, mods, carriers = graph
    p = scale(values, pmin, pmax)
    c = F32(W) / F32(SAMPLE_RATE)
    wf = F32(W)
    with np.errstate(over="ignore"):
        amp = [p[2 * j + 1] if carriers >> j & 1 else p[2 * j] * p[2 * j + 1] for j in range(ops)]
    pos = [F32(0)] * ops
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
                o[j] = F32(shape_scalar(waves[j], at(pos[j]), table) * amp[j])
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


def additive_synth_waves(waves, values, pmin, pmax, n, table, hit=None):
    """graph_synth_waves for the graphs that are sums of unmodulated carriers ("additive", "additive8": ops = len(waves)),
    with the operators as an array axis beside the rows, so that a long row costs one pass over the samples: the same
    operations on the same operands in the same order (tests/test_graph_waveforms_cpu.py holds it to graph_synth_waves).
    hit: a bool array [ops][W] in which every index that an operator reads is set"""
    ops = len(waves)
    shaped = np.stack([shape_table(w, table) for w in waves])  # [ops][W]
    p = scale(np.atleast_2d(values), pmin, pmax)
    rows = p.shape[0]
    c = F32(W) / F32(SAMPLE_RATE)
    wf = F32(W)
    f = np.ascontiguousarray(p[:, 0::2].T)  # [ops][rows]
    amp = np.ascontiguousarray(p[:, 1::2].T)
    step = c * f  # c cur with cur = f_j: the same product every sample
    pos = np.zeros((ops, rows), F32)
    which = np.arange(ops)[:, None]
    audio = np.zeros((rows, n), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(n):
            i = index_of(pos)
            o = shaped[which, i] * amp
            if hit is not None:
                hit[which, i] = True
            q = pos + step
            pos = np.where(q >= wf, q - wf, q).astype(F32)
            y = o[0]
            for j in range(1, ops):
                y = y + o[j]
            audio[:, s] = y / F32(ops) if ops > 1 else y
    return audio
