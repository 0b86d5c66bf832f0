"""The NumPy statement of sots_render_graph_genes (include/sots_hip.h), for the tests: exact, not a bound.

It is tests/_render_graph_feedback_model.py's render() with rows of D = 2 OPS + E genes and B as an array, a value per sample.
Everything of that model stands: feedback never touches a phase, so every operator's phase is the exclusive prefix sum of its
increments (cumsum in uint32), taken from genes 0 .. 2 OPS - 1 as ever.  An operator j of the mask, with q its gene column,
takes its index at sample n from the rows like every gene,

    p(n) = pmin_q + g_q(n) (pmax_q - pmin_q);  beta(n) = p(n) > 0 ? min(p(n), 2) : +0;  B(n) = beta(n) K

(g_q(n) held or glided), and ALWAYS runs the chain, also where beta(n) is +0:

    g = (h1 + h2) 0.5;  z = Phi(n) + fix(B(n) g) mod 2^32;  t(n) = shape(w, z >> 17);  h2 = h1;  h1 = t(n)

The other operators keep the fixed rule: an index other than 0 runs the chain with its constant B, 0 is feed-forward.
The chain is stated twice, as in the model of the fixed setting: chain_loop(), one sample after the other, and chain_relax(),
tiles that start from the feed-forward values and are swept until a sweep changes no bit, finished by the loop from sample
`cap` on where `cap` sweeps did not settle them.  Given the carry into a tile the chain has one solution whether B is one
number or one per sample - every sample is a function of the two before it and of its own B - and sweep k makes the first k
samples final, so both give the same bits, whatever tile and cap."""
import numpy as np

from _graph_feedback_genes_model import effective_beta, gene_operators
from _graph_feedback_model import K
from _graph_waveforms_model import GRAPHS, shape_table  # noqa: F401
from _render_continuous_model import C, F, covered, fix, genes
from _render_graph_continuous_model import scale
from _render_graph_feedback_model import bits, fix1


def chain_loop(phi, big, shaped, h1, h2):
    """t[len(phi)] and the h1, h2 it leaves: the definition, sample by sample; big[len(phi)]: B of every sample"""
    t = np.zeros(len(phi), F)
    h1, h2 = F(h1), F(h2)
    for n in range(len(phi)):
        g = F(F(h1 + h2) * F(0.5))
        z = (int(phi[n]) + fix1(F(F(big[n]) * g))) & 0xFFFFFFFF
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
        b = np.asarray(big[base:base + tile], F)
        n = len(p)
        cur = shaped[p >> 17]  # the first guess: the feed-forward values
        limit = min(cap, n)  # after n sweeps every sample of the tile is final
        settled, done = False, 0
        for _ in range(limit):
            one = np.concatenate(([h1], cur[:-1])).astype(F)
            two = np.concatenate(([h2, h1], cur[:-2])).astype(F)[:n]
            g = ((one + two).astype(F) * F(0.5)).astype(F)
            z = p + fix((b * g).astype(F))  # uint32: the word wraps
            new = shaped[z >> 17]
            done += 1
            same = np.array_equal(bits(new), bits(cur))
            cur = new
            if same:
                settled = True
                break
        capped = not settled and limit < n
        if capped:  # samples 0 .. limit - 1 are final
            rest, _, _ = chain_loop(p[limit:], b[limit:], shaped, cur[limit - 1], cur[limit - 2] if limit >= 2 else h1)
            cur = np.concatenate((cur[:limit], rest)).astype(F)
        if sweeps is not None:
            sweeps.append((done, capped))
        t[base:base + n] = cur
        h1, h2 = cur[n - 1], (cur[n - 2] if n >= 2 else h1)
    return t, F(h1), F(h2)


def render(graph, waves, beta, mask, values, pmin, pmax, tab, n, hop, glide=False, samples_per_pass=0, out_samples=None, form="loop", tile=1024,
           cap=4096, sweeps=None, betas=None):
    """out[out_samples] (default: the covered length) of values[rows][2 OPS + E].  waves: a code per operator, or None: all
    sine; beta: the fixed index per operator (0 on the mask's), or None; mask: the operators whose index is a gene.
    form: "loop" or "relax" (with tile and cap).
    sweeps: a list that receives (operator, sweeps, hit_the_cap) per tile of the relaxation.
    betas:  a dict, betas[j] becomes the list of the effective indices of gene operator j, an array per pass."""
    ops, mods, carriers = graph
    values = np.asarray(values, F).reshape(len(values), -1)
    gene_ops = gene_operators(ops, mask)
    assert values.shape[1] == 2 * ops + len(gene_ops) and 1 <= hop <= n and form in ("loop", "relax")
    waves = [0] * ops if waves is None else list(waves)
    beta = [0.0] * ops if beta is None else [float(b) for b in beta]
    assert all(beta[j] == 0 for j in gene_ops)
    shaped = [shape_table(w, tab) for w in waves]
    count = bin(carriers).count("1")
    s = covered(len(values), n, hop)
    total = s if out_samples is None else out_samples
    want = min(total, s)
    out = np.zeros(total, F)
    step = samples_per_pass if samples_per_pass else max(want, 1)
    carry = [0] * ops  # every operator's phase at the pass's start ...
    hist = [(F(0), F(0))] * ops  # ... and h1, h2 of an operator that runs the chain: all the state there is
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
                if j in gene_ops:  # always the chain, whatever the rows hold
                    eff = effective_beta(p[:, 2 * ops + gene_ops.index(j)])
                    if betas is not None:
                        betas.setdefault(j, []).append(eff)
                    big = (eff * K).astype(F)  # B(n): one fp32 product each
                elif beta[j] != 0.0:
                    big = np.full(len(idx), F(F(beta[j]) * K), F)
                else:
                    big = None
                if big is None:
                    t = shaped[j][phi >> 17]
                elif form == "loop":
                    t, h1, h2 = chain_loop(phi, big, shaped[j], hist[j][0], hist[j][1])
                    hist[j] = (h1, h2)
                else:
                    per_tile = []
                    t, h1, h2 = chain_relax(phi, big, shaped[j], hist[j][0], hist[j][1], tile, cap, per_tile)
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
