#!/usr/bin/env python3
"""What rendering feedback indices as genes costs (sots_render_graph_genes), at the shapes of 4.17: 4096 chunks
at N = 2048, hop N/4 (2 098 688 samples), `2op` and `chain3` with operator 1 feeding back, blocking calls, median of 5 after a
warm-up, legs alternating, three rounds.  A leg's spread is the largest minus the smallest of its rounds' medians.

  (a) unchanged  the calls of a context without gene operators - sots_render_graph_continuous, and sots_render_graph_feedback
                 at an index of 1 as a relaxation and serially - with this tree's library and, where --parent-root names a
                 built checkout of the commit before, with that one's, each in processes of its own, taking turns.
  (b) constant   a gene operator whose range is [b, b] against the fixed index b, b = 0.25, 1, 1.5, 2, relaxation and serial.
  (c) varying    a gene range of [0, 2] with a random gene per row: the library's choice (the relaxation) against the serial
                 form - what the rule "a gene operator is relaxed" (graph_genes_form, csrc/sots_rules.h) rests on.

    python tools/render_graph_genes_bench.py [--out profiles/r31_render_graph_genes.json] [--parent-root DIR] [--chunks 4096] [--reps 5]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd"
N, HOP, OP = 2048, 512, 1
GRAPHS = {"2op": (2, [0, 0b1], 0b10), "chain3": (3, [0, 0b1, 0b10], 0b100)}
BETAS = [0.25, 1.0, 1.5, 2.0]
ROUNDS = 3
SERIAL, RELAX = 1, 2


def ranges(graph, gene=None):
    """frequencies to 3520 Hz, modulation indices to 8, carrier levels to 1; gene: the range of the one feedback gene"""
    ops, _, carriers = graph
    pmax = []
    for j in range(ops):
        pmax += [3520.0, 1.0 if carriers >> j & 1 else 8.0]
    pmin = [0.0] * (2 * ops)
    return (pmin + [gene[0]], pmax + [gene[1]]) if gene else (pmin, pmax)


def rows_of(ops, chunks, gene=False):
    v = np.random.default_rng(27 + ops).uniform(0.05, 0.95, (chunks, 2 * ops)).astype(np.float32)
    if gene:
        v = np.concatenate([v, np.random.default_rng(31 + ops).random((chunks, 1), dtype=np.float32)], axis=1)
    return v


def context(pkg, graph, gene=None):
    pmin, pmax = ranges(graph, gene)
    kw = dict(feedback_genes=1 << OP) if gene else {}
    return pkg.HipES(32, 32, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=11, param_min=pmin, param_max=pmax, seed=1, workgroup_size=32,
                     graph=pkg.capi.make_voice_graph(*graph), **kw)


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def medians(legs, reps):
    """{leg: median ms} of `reps` timed calls per leg after one warm-up each, the legs taking turns"""
    for call in legs.values():
        call()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, call in legs.items():
            times[k].append(timed(call))
    return {k: float(np.median(v)) for k, v in times.items()}


def fixed_index(ops, b):
    index = [0.0] * ops
    index[OP] = b
    return index


def unchanged(root, chunks, reps):
    """one round of (a) with the package under `root`: {graph: {leg: median ms}}"""
    sys.path.insert(0, root)
    pkg = importlib.import_module(PKG)
    out = {}
    for name, graph in GRAPHS.items():
        ops = graph[0]
        values = rows_of(ops, chunks)
        plain, fed = context(pkg, graph), context(pkg, graph)
        fed.set_voice_feedback(fixed_index(ops, 1.0))
        out[name] = medians({"graph_continuous": lambda: plain.render_graph_continuous(values, HOP),
                             "graph_feedback_relax": lambda: fed.render_graph_feedback(values, HOP, chain_form=RELAX),
                             "graph_feedback_serial": lambda: fed.render_graph_feedback(values, HOP, chain_form=SERIAL)}, reps)
        plain.close()
        fed.close()
    return out


def spread(per_round):
    return {"rounds": [round(x, 3) for x in per_round], "median": float(np.median(per_round)), "spread": float(max(per_round) - min(per_round))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_render_graph_genes.json"))
    ap.add_argument("--parent-root", default=None, help="a built checkout of the commit before: leg (a) runs its library too")
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--unchanged-worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.unchanged_worker:
        print(json.dumps(unchanged(a.unchanged_worker, a.chunks, a.reps)))
        return
    result = {"shape": {"N": N, "hop": HOP, "chunks": a.chunks, "samples": (a.chunks - 1) * HOP + N, "reps": a.reps, "rounds": ROUNDS,
                        "feedback_operator": OP},
              "unit": "ms per blocking call; per leg the rounds' medians, their median and their spread (max - min)"}

    # ---- (a) a context without gene operators: the parent's library and this tree's, in processes that take turns ----
    sides = {"this_tree": ROOT}
    if a.parent_root:
        sides = {"parent": os.path.abspath(a.parent_root), "this_tree": ROOT}
    runs = {side: [] for side in sides}
    for _ in range(ROUNDS):
        for side, root in sides.items():
            cmd = [sys.executable, os.path.abspath(__file__), "--unchanged-worker", root, "--chunks", str(a.chunks), "--reps", str(a.reps)]
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
            if done.returncode != 0:
                raise SystemExit("leg (a), %s: %s" % (side, done.stderr[-2000:]))
            runs[side].append(json.loads(done.stdout.strip().splitlines()[-1]))
    result["unchanged"] = []
    for name in GRAPHS:
        for leg in runs["this_tree"][0][name]:
            row = {"graph": name, "call": leg}
            for side in sides:
                row[side] = spread([r[name][leg] for r in runs[side]])
            if a.parent_root:
                row["this_tree_minus_parent"] = row["this_tree"]["median"] - row["parent"]["median"]
                row["within_parents_spread"] = bool(abs(row["this_tree_minus_parent"]) <= row["parent"]["spread"])
            result["unchanged"].append(row)
            print(json.dumps(row), flush=True)

    sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    # ---- (b) a gene whose range is [b, b] against the fixed index b ----
    result["constant"] = []
    for name, graph in GRAPHS.items():
        ops = graph[0]
        values = rows_of(ops, a.chunks, gene=True)
        narrow = np.ascontiguousarray(values[:, :2 * ops])
        for b in BETAS:
            gene, fixed = context(pkg, graph, gene=(b, b)), context(pkg, graph)
            fixed.set_voice_feedback(fixed_index(ops, b))
            legs = {"fixed_relax": lambda: fixed.render_graph_feedback(narrow, HOP, chain_form=RELAX),
                    "gene_relax": lambda: gene.render_graph_genes(values, HOP, chain_form=RELAX),
                    "fixed_serial": lambda: fixed.render_graph_feedback(narrow, HOP, chain_form=SERIAL),
                    "gene_serial": lambda: gene.render_graph_genes(values, HOP, chain_form=SERIAL)}
            assert gene.render_graph_genes(values, HOP, chain_form=RELAX).tobytes() == fixed.render_graph_feedback(narrow, HOP, chain_form=RELAX).tobytes()
            rounds = [medians(legs, a.reps) for _ in range(ROUNDS)]
            row = {"graph": name, "beta": b}
            row.update({k: spread([r[k] for r in rounds]) for k in legs})
            for form in ("relax", "serial"):
                row["gene_over_fixed_" + form] = row["gene_" + form]["median"] / row["fixed_" + form]["median"]
            result["constant"].append(row)
            print(json.dumps(row), flush=True)
            gene.close()
            fixed.close()

    # ---- (c) a gene per row anywhere in [0, 2]: the library's choice against the serial form ----
    result["varying"] = []
    for name, graph in GRAPHS.items():
        ops = graph[0]
        values = rows_of(ops, a.chunks, gene=True)
        es = context(pkg, graph, gene=(0.0, 2.0))
        legs = {"library": lambda: es.render_graph_genes(values, HOP, chain_form=0),
                "serial": lambda: es.render_graph_genes(values, HOP, chain_form=SERIAL),
                "library_glide": lambda: es.render_graph_genes(values, HOP, glide=True, chain_form=0),
                "serial_glide": lambda: es.render_graph_genes(values, HOP, glide=True, chain_form=SERIAL)}
        assert legs["library"]().tobytes() == legs["serial"]().tobytes()
        rounds = [medians(legs, a.reps) for _ in range(ROUNDS)]
        row = {"graph": name, "gene_range": [0.0, 2.0]}
        row.update({k: spread([r[k] for r in rounds]) for k in legs})
        row["library_over_serial"] = row["library"]["median"] / row["serial"]["median"]
        row["library_over_serial_glide"] = row["library_glide"]["median"] / row["serial_glide"]["median"]
        result["varying"].append(row)
        print(json.dumps(row), flush=True)
        es.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
