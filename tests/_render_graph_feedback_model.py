"""The NumPy statement of sots_render_graph_feedback (include/sots_hip.h), for the tests: exact, not a bound.

Everything of tests/_render_graph_continuous_model.py stands: feedback never touches a phase, so every operator's phase is
still the exclusive prefix sum of its increments (cumsum in uint32).  An operator with beta_j != 0 turns its finished phase
words and B_j = beta_j K into its shaped values by a chain over the samples,

    g = (h1 + h2) 0.5;  z = Phi(n) + fix(B g) mod 2^32;  t(n) = shape(w, z >> 17);  h2 = h1;  h1 = t(n)

with h1 = h2 = +0 at sample 0 of the rendering.  The chain is stated twice: chain_loop(), one sample after the other, and
chain_relax(), which starts a tile from the feed-forward values shape(w, Phi >> 17) and recomputes every sample from its two
predecessors in the previous sweep, all at once, until a sweep changes no bit; after `cap` sweeps the tile is finished by the
loop from sample `cap` on (sweep k makes at least the first k samples final).  The chain has one solution - the carry is given
and every sample is a function of the two before it - so both give the same bits, whatever tile and cap."""
import numpy as np

from _graph_feedback_model import K
from _graph_waveforms_model import GRAPHS, shape_table  # noqa: F401
from _render_continuous_model import C, F, SCALE, covered, fix, genes
from _render_graph_continuous_model import W, scale


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def fix1(x):
    """fix() of one fp32 number as a Python int (|x 2^17| is far below 2^62 for an offset)"""
    return int(np.rint(F(F(x) * SCALE)))


def chain_loop(phi, big, shaped, h1, h2, note=None):
    """t[len(phi)] and the h1, h2 it leaves: the definition, sample by sample"""
    t = np.zeros(len(phi), F)
    h1, h2 = F(h1), F(h2)
    for n in range(len(phi)):
        g = F(F(h1 + h2) * F(0.5))
        off = fix1(F(big * g))
        z = (int(phi[n]) + off) & 0xFFFFFFFF
        if note is not None:
            note(z >> 17, off)
        v = shaped[z >> 17]
        t[n] = v
        h2, h1 = h1, v
    return t, h1, h2


def chain_relax(phi, big, shaped, h1, h2, tile, cap, sweeps=None):
    """the same by relaxation in tiles of `tile` samples; sweeps: a list that receives (sweeps, hit_the_cap) per tile"""
    assert tile >= 1 and cap >= 1
    t = np.zeros(len(phi), F)
    h1, h2 = F(h1), F(h2)
    for base in range(0, len(phi), tile):
        p = np.asarray(phi[base:base + tile], np.uint32)
        n = len(p)
        cur = shaped[p >> 17]  # the first guess: the feed-forward values
        limit = min(cap, n)  # after n sweeps every sample of the tile is final
        settled, done = False, 0
        for _ in range(limit):
            a = np.concatenate(([h1], cur[:-1])).astype(F)
            b = np.concatenate(([h2, h1], cur[:-2])).astype(F)[:n]
            g = ((a + b).astype(F) * F(0.5)).astype(F)
            z = p + fix((F(big) * g).astype(F))  # uint32: the word wraps
            new = shaped[z >> 17]
            done += 1
            same = np.array_equal(bits(new), bits(cur))
            cur = new
            if same:
                settled = True
                break
        capped = not settled and limit < n
        if capped:  # samples 0 .. limit - 1 are final
            rest, _, _ = chain_loop(p[limit:], big, shaped, cur[limit - 1], cur[limit - 2] if limit >= 2 else h1)
            cur = np.concatenate((cur[:limit], rest)).astype(F)
        if sweeps is not None:
            sweeps.append((done, capped))
        t[base:base + n] = cur
        h1, h2 = cur[n - 1], (cur[n - 2] if n >= 2 else h1)
    return t, F(h1), F(h2)


def render(graph, waves, beta, values, pmin, pmax, tab, n, hop, glide=False, samples_per_pass=0, out_samples=None, form="loop", tile=1024,
           cap=4096, sweeps=None, seen=None, signs=None):
    """out[out_samples] (default: the covered length).  waves: a code per operator, or None: all sine; beta: an index per
    operator, or None: no feedback.  form: "loop" or "relax" (with tile and cap).
    sweeps: a list that receives (operator, sweeps, hit_the_cap) per tile of the relaxation.
    seen:   a dict, seen[code] becomes the set of index regions (z >> 17) // (W/8) that a feedback operator of that code read.
    signs:  a set that receives -1, 0, 1: the signs of the offsets fix(B g) that occurred (loop form only)."""
    ops, mods, carriers = graph
    values = np.asarray(values, F).reshape(len(values), -1)
    assert values.shape[1] == 2 * ops and 1 <= hop <= n and form in ("loop", "relax")
    waves = [0] * ops if waves is None else list(waves)
    beta = [0.0] * ops if beta is None else [float(b) for b in beta]
    shaped = [shape_table(w, tab) for w in waves]
    big = [F(F(b) * K) for b in beta]  # B_j: one fp32 product
    count = bin(carriers).count("1")
    s = covered(len(values), n, hop)
    total = s if out_samples is None else out_samples
    want = min(total, s)
    out = np.zeros(total, F)
    step = samples_per_pass if samples_per_pass else max(want, 1)
    carry = [0] * ops  # every operator's phase at the pass's start ...
    hist = [(F(0), F(0))] * ops  # ... and h1, h2 of a feedback operator: all the state there is
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
                inc = fix(C * cur)
                incl = np.cumsum(inc, dtype=np.uint32)
                phi = np.uint32(carry[j]) + incl - inc  # exclusive: the phase BEFORE this sample's update
                carry[j] = (carry[j] + int(incl[-1])) & 0xFFFFFFFF
                if beta[j] == 0.0:
                    t = shaped[j][phi >> 17]
                elif form == "loop":
                    note = None
                    if seen is not None or signs is not None:
                        def note(at, off, w=waves[j]):
                            if seen is not None:
                                seen.setdefault(w, set()).add(at // (W // 8))
                            if signs is not None:
                                signs.add((off > 0) - (off < 0))
                    t, h1, h2 = chain_loop(phi, big[j], shaped[j], hist[j][0], hist[j][1], note)
                    hist[j] = (h1, h2)
                else:
                    per_tile = []
                    t, h1, h2 = chain_relax(phi, big[j], shaped[j], hist[j][0], hist[j][1], tile, cap, per_tile)
                    hist[j] = (h1, h2)
                    if sweeps is not None:
                        sweeps.extend((j, d, c) for d, c in per_tile)
                o[j] = t * (a if carriers >> j & 1 else f * a)
            y = None
            for j in range(ops):
                if carriers >> j & 1:
                    y = o[j] if y is None else y + o[j]
            out[idx] = y / F(count) if count > 1 else y
    return out
