"""The NumPy statement of sots_render_continuous (include/sots_hip.h), for the tests: exact, not a bound.

The track is ONE voice whose oscillators never restart.  Phases are uint32 words, unsigned 15.17 fixed point, so an
operator's phase is the exclusive prefix sum of its increments, mod 2^32: np.cumsum(dtype=uint32).  Integer addition is
associative, so the sum is the same bits however the device tiles it.  Everything in front of the sum is per sample and
fp32, one rounding per operation: the row position, the genes (held or interpolated), the parameters and the CPU oracle's
expressions (oracle/sots_oracle.c:130-215).

render() is the vectorised form, pass by pass with carried phases; render_loop() is a plain per-sample loop that exists
only to check the vectorised form on the CPU."""
import numpy as np

F = np.float32
C = F(32768.0) / F(44100.0)  # w2srRatio in fp32
SCALE = F(131072.0)  # 2^17
SHAPE = {0: (2, 1, 4), 1: (3, 1, 6), 2: (2, 3, 12), 3: (4, 1, 8)}  # kind -> (operators per chain, chains, genes)


PMAX = {0: [3520.0, 8.0, 3520.0, 1.0], 1: [3520.0, 8.0] * 3, 2: [3520.0, 8.0, 3520.0, 1.0], 3: [3520.0, 8.0] * 4}  # the tests' parameter box
DIMS = {kind: shape[2] for kind, shape in SHAPE.items()}


def track_rows(kind, rows, seed):
    """the rows of genes the tests render: random in [0.05, 0.95), nothing at a bound, with the corners of the box PMAX that
    make the largest and the most negative modulated increments put in by hand"""
    v = np.random.default_rng(seed).uniform(0.05, 0.95, (rows, DIMS[kind])).astype(F)
    if rows >= 3:
        v[1] = 0.95  # everything high: cur up to 0.95 * 0.95 * 28160 + 3344 Hz, beyond the Nyquist rate
        v[2] = 0.95
        v[2][3 if kind in (1, 3) else 2] = 0.05  # a low offset under a high index: cur swings far below zero
    return v


def covered(rows, n, hop):
    return (rows - 1) * hop + n


def positions(idx, n, hop, rows):
    """row k and the r samples behind its anchor k hop + N/2, for the sample numbers idx"""
    m = np.asarray(idx, np.int64) - n // 2
    pos = m > 0
    k = np.where(pos, m // hop, 0)
    r = np.where(pos, m % hop, 0)
    end = k >= rows - 1
    return np.where(end, rows - 1, k), np.where(end, 0, r)


def genes(values, idx, n, hop, glide):
    """g[len(idx)][D]: the genes at the samples idx"""
    values = np.asarray(values, F)
    k, r = positions(idx, n, hop, len(values))
    if not glide:
        return values[k + (2 * r >= hop)]
    t = (r.astype(F) / F(hop))[:, None]  # fp32 / fp32: correctly rounded
    a, b = values[k], values[np.minimum(k + 1, len(values) - 1)]
    return np.where((r == 0)[:, None], a, a + t * (b - a))


def params(kind, g, pmin, pmax):
    d = SHAPE[kind][2]
    sc = np.arange(d) & 3 if kind == 2 else np.arange(d)  # the triple voice scales all three chains by entries 0..3
    lo, hi = np.asarray(pmin, F)[sc], np.asarray(pmax, F)[sc]
    return lo + g * (hi - lo)


def terms(kind, p):
    """per chain: (the first operator's increment in table entries, [(mul, off) of operators 1 ...], output gain)"""
    ops, chains, _ = SHAPE[kind]
    out = []
    for j in range(chains):
        if kind in (0, 2):
            b = 4 * j
            out.append((C * p[..., b], [(p[..., b] * p[..., b + 1], p[..., b + 2])], p[..., b + 3]))
        else:
            out.append((C * p[..., 1], [(p[..., 2 * o - 2] * p[..., 2 * o - 1], p[..., 2 * o + 1]) for o in range(1, ops)],
                        p[..., 2 * ops - 2] * p[..., 2 * ops - 1]))
    return out


def fix_wide(x):
    """rint(x 2^17) as int64 BEFORE the reduction mod 2^32; 0 where |x 2^17| < 2^62 does not hold"""
    y = np.asarray(x, F) * SCALE
    ok = np.abs(y) < F(2.0 ** 62)
    return np.rint(np.where(ok, y, F(0))).astype(np.int64)


def fix(x):
    return (fix_wide(x) & 0xFFFFFFFF).astype(np.uint32)


def render(kind, values, pmin, pmax, tab, n, hop, glide=False, samples_per_pass=0, out_samples=None, wide=None):
    """out[out_samples] (default: the covered length).  wide: a list that receives every stage's increments before their
    reduction (int64 arrays), for the tests that look at what the inputs cover."""
    values = np.asarray(values, F).reshape(len(values), -1)
    ops, chains, d = SHAPE[kind]
    assert values.shape[1] == d and 1 <= hop <= n
    tab = np.asarray(tab, F)
    s = covered(len(values), n, hop)
    total = s if out_samples is None else out_samples
    want = min(total, s)
    out = np.zeros(total, F)
    step = samples_per_pass if samples_per_pass else max(want, 1)
    carry = [[0] * ops for _ in range(chains)]  # every operator's phase at the pass's start: all the state there is
    for s0 in range(0, want, step):
        idx = np.arange(s0, min(s0 + step, want))
        tm = terms(kind, params(kind, genes(values, idx, n, hop, glide), pmin, pmax))
        acc = None
        for j, (inc0, mods, gain) in enumerate(tm):
            phi = None
            for o in range(ops):
                x = inc0 if o == 0 else C * (tab[phi >> 17] * mods[o - 1][0] + mods[o - 1][1])
                if wide is not None:
                    wide.append(fix_wide(x))
                inc = fix(x)
                incl = np.cumsum(inc, dtype=np.uint32)
                phi = np.uint32(carry[j][o]) + incl - inc  # exclusive: the phase BEFORE this sample's update
                carry[j][o] = (carry[j][o] + int(incl[-1])) & 0xFFFFFFFF
            tot = tab[phi >> 17] * gain
            acc = tot if acc is None else acc + tot
        out[idx] = acc / F(3.0) if chains == 3 else acc
    return out


def render_loop(kind, values, pmin, pmax, tab, n, hop, glide=False, out_samples=None):
    """the same, one sample after the other with every operator's phase carried in a Python int"""
    values = np.asarray(values, F).reshape(len(values), -1)
    ops, chains, d = SHAPE[kind]
    rows = len(values)
    s = covered(rows, n, hop)
    total = s if out_samples is None else out_samples
    out = np.zeros(total, F)
    pmin, pmax = np.asarray(pmin, F), np.asarray(pmax, F)
    phase = [[0] * ops for _ in range(chains)]
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
        p = [F(pmin[e & 3 if kind == 2 else e] + F(g[e] * F(pmax[e & 3 if kind == 2 else e] - pmin[e & 3 if kind == 2 else e]))) for e in range(d)]
        tots = []
        for j in range(chains):
            if kind in (0, 2):
                b = 4 * j
                inc0, mods, gain = F(C * p[b]), [(F(p[b] * p[b + 1]), p[b + 2])], p[b + 3]
            else:
                inc0 = F(C * p[1])
                mods = [(F(p[2 * o - 2] * p[2 * o - 1]), p[2 * o + 1]) for o in range(1, ops)]
                gain = F(p[2 * ops - 2] * p[2 * ops - 1])
            before = [ph for ph in phase[j]]  # every operator reads the one in front of it before that one's update
            for o in range(ops):
                x = inc0 if o == 0 else F(C * F(F(tab[before[o - 1] >> 17] * mods[o - 1][0]) + mods[o - 1][1]))
                y = F(x * SCALE)
                step = int(np.rint(y)) if abs(float(y)) < 2.0 ** 62 else 0
                phase[j][o] = (before[o] + step) % (1 << 32)
            tots.append(F(tab[before[ops - 1] >> 17] * gain))
        out[i] = F(F(F(tots[0] + tots[1]) + tots[2]) / F(3.0)) if chains == 3 else tots[0]
    return out


def interior_rms(x, n):
    """RMS over the interior of a rendering: a window length off either end"""
    x = np.asarray(x, np.float64)[n:-n]
    return float(np.sqrt(np.mean(x * x)))
