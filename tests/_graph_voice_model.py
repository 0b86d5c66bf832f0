"""The operator-graph voice (SOTS_SYNTH_GRAPH, include/sots_hip.h) in NumPy: the definition, operation by operation, on
float32 arrays - vectorised over rows, loops over samples and operators only.  graph_synth() is what the GPU tests compare
the kernel against bit for bit; graph_synth_scalar() restates it row by row with NumPy float32 scalars."""
import numpy as np

W = 32768
SAMPLE_RATE = 44100
F32 = np.float32

# the graphs the tests use: (operators, modulators as masks, carriers as a mask)
GRAPHS = {
    "2op": (2, [0, 0b1], 0b10),                                       # the 2-op voice
    "triple": (6, [0, 0b1, 0, 0b100, 0, 0b10000], 0b101010),          # the triple voice: three pairs, three carriers
    "chain3": (3, [0, 0b1, 0b10], 0b100),                             # 0 -> 1 -> 2
    "two_mods": (3, [0, 0, 0b011], 0b100),                            # 0 and 1 into 2: the order of the sum
    "one_mod_two_carriers": (3, [0, 0b1, 0b1], 0b110),                # 0 into 1 and into 2
    "additive": (2, [0, 0], 0b11),                                    # two unmodulated carriers
    "chain8": (8, [0] + [1 << (j - 1) for j in range(1, 8)], 1 << 7), # D = 16
    "fan3": (4, [0, 0, 0, 0b0111], 0b1000),                           # 4 operators: a sum of three
    "stacks5": (5, [0, 0b1, 0b10, 0, 0b1000], 0b10100),               # 5 operators, D = 10: a chain of three and a pair
    "seven": (7, [0, 0b1, 0b10, 0, 0, 0, 0b0111000], 0b1000100),      # 7 operators, D = 14: a chain beside a fan
    "dense8": (8, [0] + [(1 << min(j, 6)) - 1 for j in range(1, 8)], 0b11000000),  # every modulator into everything after it: fan-in 6
    "additive8": (8, [0] * 8, 0xFF),                                  # a sum of eight and a division by 8
    "one_to_seven": (8, [0] + [1] * 7, 0xFE),                         # one output read by seven operators
}


def scale(values, pmin, pmax):
    """p_g = pmin_g + v_g (pmax_g - pmin_g), fp32; no folding of the ranges"""
    v = np.asarray(values, F32)
    d = v.shape[-1]
    lo, hi = np.asarray(pmin, F32)[:d], np.asarray(pmax, F32)[:d]
    return lo + v * (hi - lo)


def tab_at(table, pos):
    """table[clamp((int)pos, 0, W-1)], decided on the float: at or beyond W -> W-1, negative or NaN -> 0"""
    with np.errstate(invalid="ignore"):
        idx = np.where(pos >= F32(W), F32(W - 1), np.where(pos > F32(0), pos, F32(0)))
    return table[idx.astype(np.int64)]


def graph_synth(graph, values, pmin, pmax, n, table, seen=None):
    """audio[rows][n] of values[rows][2 OPS].  seen: a dict that is told whether any operator output and any phase was
    infinite or NaN (keys output_inf, output_nan, phase_inf, phase_nan)"""
    ops, mods, carriers = graph
    p = scale(np.atleast_2d(values), pmin, pmax)
    rows = p.shape[0]
    table = np.asarray(table, F32)
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
                o[j] = tab_at(table, pos[j]) * amp[j]
                cur = None
                for i in range(j):
                    if mods[j] >> i & 1:
                        cur = o[i] if cur is None else cur + o[i]
                cur = f[j] if cur is None else cur + f[j]
                q = pos[j] + c * cur
                q = np.where(q >= wf, q - wf, q)
                if mods[j]:
                    q = np.where(q < F32(0), q + wf, q)
                pos[j] = q.astype(F32)
                if seen is not None:
                    for key, x, test in (("output_inf", o[j], np.isinf), ("output_nan", o[j], np.isnan),
                                         ("phase_inf", pos[j], np.isinf), ("phase_nan", pos[j], np.isnan)):
                        seen[key] = seen.get(key, False) or bool(test(x).any())
            y = None
            for j in range(ops):
                if carriers >> j & 1:
                    y = o[j] if y is None else y + o[j]
            audio[:, s] = y / F32(count) if count > 1 else y
    return audio


def graph_synth_scalar(graph, values, pmin, pmax, n, table):
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
            return table[W - 1]
        if not x > F32(0):
            return table[0]
        return table[int(x)]

    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(n):
            o = [F32(0)] * ops
            for j in range(ops):
                o[j] = F32(at(pos[j]) * amp[j])
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


def edge_rows(d, rows, seed):
    """values[rows][d] in [0, 1): random rows with a row of all 0 and a row of all 1 in front"""
    rng = np.random.default_rng(seed)
    v = rng.random((rows, d), dtype=np.float32)
    v[0] = 0.0
    if rows > 1:
        v[1] = 1.0
    return v


def ranges(ops, negative=True, strong=True):
    """(pmin, pmax) of 2 OPS genes: frequencies up to 3520 Hz, from a negative minimum where asked (phases go below 0);
    indices up to 8, or up to 64 where `strong` - 3520 x 64 x 0.743 = 167 000 table steps per sample, several times W, so a
    modulated phase overshoots by more than W in either direction and the index is clamped"""
    pmin, pmax = [], []
    for j in range(ops):
        pmin += [-880.0 if negative else 0.0, -2.0 if negative else 0.0]
        pmax += [3520.0, 64.0 if strong and j == 0 else 8.0]
    return pmin, pmax


def overflow_ranges(ops):
    """ranges(ops) with operator 0's maxima at 3e19: its genes are finite, its level f * a is +inf in fp32 wherever
    v_0 v_1 > 0.38, so its output is NaN at a table entry of 0 (the first sample) and +-inf elsewhere, and the phases of what
    it modulates are not finite.  The index is clamped on the float, so such a phase reads entry W-1 or 0 and nothing else;
    operator 0 is never a carrier, so the audio stays finite"""
    pmin, pmax = ranges(ops)
    pmax[0] = pmax[1] = 3e19
    return pmin, pmax
