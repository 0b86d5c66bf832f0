"""The NumPy statement of sots_render_graph_continuous (include/sots_hip.h), for the tests: exact, not a bound.

The parameter track of an operator-graph voice as ONE voice whose oscillators never restart.  Row position, HOLD / GLIDE,
fix() and the covered length are those of sots_render_continuous and are taken from tests/_render_continuous_model.py; the
graphs, their scaling and the shape tables are those of the graph voice (tests/_graph_voice_model.py,
tests/_graph_waveforms_model.py).  Every operator's phase is a uint32 word, unsigned 15.17 fixed point, and the exclusive
prefix sum of its increments mod 2^32; operator j's increment at sample n reads the phases at n of the operators i < j that
modulate it, so the operators are taken in ascending j.  There is no feedback here: the call refuses it.

render() is the vectorised form, pass by pass with carried phases; render_loop() is a plain per-sample loop with the phases
in Python ints that exists only to check the vectorised form on the CPU."""
import numpy as np

from _graph_waveforms_model import GRAPHS, shape_scalar, shape_table  # noqa: F401
from _render_continuous_model import C, F, SCALE, covered, fix, fix_wide, genes, interior_rms  # noqa: F401

W = 32768


def scale(g, pmin, pmax):
    """p_g = pmin_g + g_g (pmax_g - pmin_g), fp32, gene by gene: no folding of the ranges"""
    d = g.shape[-1]
    lo, hi = np.asarray(pmin, F)[:d], np.asarray(pmax, F)[:d]
    return lo + g * (hi - lo)


def graph_rows(ops, rows, seed):
    """the rows of genes the tests render: random in [0.05, 0.95), nothing at a bound, with two corner rows put in by hand -
    everything high (under ranges(): operator 0's level f a reaches 3300 x 60 Hz, increments of many times 2^31 before
    the reduction) and everything high over the lowest frequencies (below zero under ranges(): negative increments)"""
    v = np.random.default_rng(seed).uniform(0.05, 0.95, (rows, 2 * ops)).astype(F)
    if rows >= 3:
        v[1] = 0.95
        v[2] = 0.95
        v[2][0::2] = 0.05
    return v


# the waveform settings the tests render
MIXED8 = [3, 1, 6, 0, 7, 4, 2, 5]  # one of every code on the eight operators of dense8


def chain3_waves(w):
    """code w once as a modulator (operator 0) and once as the carrier (operator 2) of chain3"""
    return [w, 0, w]


def audible_ranges(graph):
    """(pmin, pmax) as the fixed voices' tests have them: frequencies to 3520 Hz, modulation indices to 8, carrier levels to 1"""
    ops, _, carriers = graph
    pmax = []
    for j in range(ops):
        pmax += [3520.0, 1.0 if carriers >> j & 1 else 8.0]
    return [0.0] * (2 * ops), pmax


def levels(graph):
    """level(j) = 0 for an unmodulated operator, else 1 + the largest level among its modulators"""
    ops, mods, _ = graph
    lv = []
    for j in range(ops):
        lv.append(0 if mods[j] == 0 else 1 + max(lv[i] for i in range(j) if mods[j] >> i & 1))
    return lv


def render(graph, waves, values, pmin, pmax, tab, n, hop, glide=False, samples_per_pass=0, out_samples=None, wide=None, seen=None):
    """out[out_samples] (default: the covered length).  waves: a code per operator, or None: all sine.
    wide: a list that receives (operator, its increments before the reduction mod 2^32 as int64, cur) per pass.
    seen: a dict, seen[(code, "modulator" | "carrier")] becomes the set of index regions i // (W/8) that were read."""
    ops, mods, carriers = graph
    values = np.asarray(values, F).reshape(len(values), -1)
    assert values.shape[1] == 2 * ops and 1 <= hop <= n
    waves = [0] * ops if waves is None else list(waves)
    shaped = [shape_table(w, tab) for w in waves]
    count = bin(carriers).count("1")
    s = covered(len(values), n, hop)
    total = s if out_samples is None else out_samples
    want = min(total, s)
    out = np.zeros(total, F)
    step = samples_per_pass if samples_per_pass else max(want, 1)
    carry = [0] * ops  # every operator's phase at the pass's start: all the state there is
    with np.errstate(over="ignore", invalid="ignore"):
        for s0 in range(0, want, step):
            idx = np.arange(s0, min(s0 + step, want))
            p = scale(genes(values, idx, n, hop, glide), pmin, pmax)
            o = [None] * ops
            for j in range(ops):
                f, a = p[:, 2 * j], p[:, 2 * j + 1]
                cur = None
                for i in range(j):
                    if mods[j] >> i & 1:
                        cur = o[i] if cur is None else cur + o[i]
                cur = f if cur is None else cur + f
                x = C * cur
                inc = fix(x)
                if wide is not None:
                    wide.append((j, fix_wide(x), cur))
                incl = np.cumsum(inc, dtype=np.uint32)
                phi = np.uint32(carry[j]) + incl - inc  # exclusive: the phase BEFORE this sample's update
                carry[j] = (carry[j] + int(incl[-1])) & 0xFFFFFFFF
                at = phi >> 17
                if seen is not None:
                    key = (waves[j], "carrier" if carriers >> j & 1 else "modulator")
                    seen.setdefault(key, set()).update(np.unique(at // (W // 8)).tolist())
                o[j] = shaped[j][at] * (a if carriers >> j & 1 else f * a)
            y = None
            for j in range(ops):
                if carriers >> j & 1:
                    y = o[j] if y is None else y + o[j]
            out[idx] = y / F(count) if count > 1 else y
    return out


def render_loop(graph, waves, values, pmin, pmax, tab, n, hop, glide=False, out_samples=None):
    """the same, one sample after the other: NumPy float32 scalars, every operator's phase carried in a Python int, the
    definition's own if-statements for the shapes"""
    ops, mods, carriers = graph
    values = np.asarray(values, F).reshape(len(values), -1)
    rows, d = len(values), 2 * ops
    waves = [0] * ops if waves is None else list(waves)
    tab = np.asarray(tab, F)
    pmin, pmax = np.asarray(pmin, F), np.asarray(pmax, F)
    count = bin(carriers).count("1")
    s = covered(rows, n, hop)
    total = s if out_samples is None else out_samples
    out = np.zeros(total, F)
    phase = [0] * ops
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(min(total, s)):
            m = i - n // 2
            k, r = (m // hop, m % hop) if m > 0 else (0, 0)
            if k >= rows - 1:
                k, r = rows - 1, 0
            if not glide:
                g = values[k + (1 if 2 * r >= hop else 0)]
            elif r == 0:
                g = values[k]
            else:
                t = F(F(r) / F(hop))
                g = np.array([F(values[k][e] + F(t * F(values[k + 1][e] - values[k][e]))) for e in range(d)], F)
            p = [F(pmin[e] + F(g[e] * F(pmax[e] - pmin[e]))) for e in range(d)]
            o = [F(0)] * ops
            for j in range(ops):
                f, a = p[2 * j], p[2 * j + 1]
                amp = a if carriers >> j & 1 else F(f * a)
                o[j] = F(shape_scalar(waves[j], phase[j] >> 17, tab) * amp)
                ins = [o[q] for q in range(j) if mods[j] >> q & 1]
                if ins:
                    cur = ins[0]
                    for x in ins[1:]:
                        cur = F(cur + x)
                    cur = F(cur + f)
                else:
                    cur = f
                y = F(F(C * cur) * SCALE)
                inc = int(np.rint(y)) if abs(float(y)) < 2.0 ** 62 else 0  # (NaN fails the comparison)
                phase[j] = (phase[j] + inc) % (1 << 32)
            heard = [o[j] for j in range(ops) if carriers >> j & 1]
            y = heard[0]
            for x in heard[1:]:
                y = F(y + x)
            out[i] = F(y / F(count)) if count > 1 else y
    return out
