#!/usr/bin/env python3
"""What feedback costs the phase-continuous rendering of the graph voice, and which form of the chain is
faster where: 4096 chunks at N = 2048, hop N/4 (2 098 688 samples), blocking calls, median of 5 after a warm-up, legs
alternating.  For `2op` (feedback on the carrier) and `chain3` (feedback on operator 1) at beta = 0.25 .. 2: the serial form,
the relaxation with caps 64, 256 and 1024, the same graph without feedback through sots_render_graph_continuous (the price of
feedback) and sots_render_overlap_add on the same context.  "relax_wins": the relaxation (at its best cap) beat the serial form
in EVERY repetition - the only indices for which graph_feedback_form (csrc/sots_rules.h) may choose it.

    python tools/render_graph_feedback_bench.py [--out profiles/r27_render_graph_feedback.json] [--chunks 4096] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _render_graph_continuous_model as GM  # noqa: E402

BETAS = [0.25, 0.5, 0.75, 1.0, 1.5, 2.0]
CAPS = [64, 256, 1024]
CASES = {"2op": 1, "chain3": 1}  # graph -> the operator that feeds back


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_render_graph_feedback.json"))
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import importlib
    pkg = importlib.import_module("survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
    n, hop = 2048, 512
    result = {"shape": {"N": n, "hop": hop, "chunks": a.chunks, "samples": (a.chunks - 1) * hop + n, "reps": a.reps}, "unit": "ms per call, median",
              "cases": []}
    for name, op in CASES.items():
        graph = GM.GRAPHS[name]
        ops = graph[0]
        pmin, pmax = GM.audible_ranges(graph)
        values = np.random.default_rng(27 + ops).uniform(0.05, 0.95, (a.chunks, 2 * ops)).astype(np.float32)
        es = pkg.HipES(32, 32, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=11, param_min=pmin, param_max=pmax, seed=1, workgroup_size=32,
                       graph=pkg.capi.make_voice_graph(*graph))
        for beta in BETAS:
            index = [0.0] * ops
            index[op] = beta
            legs = {"serial": lambda: es.render_graph_feedback(values, hop, chain_form=1)}
            for cap in CAPS:
                legs["relax_%d" % cap] = lambda cap=cap: es.render_graph_feedback(values, hop, chain_form=2, relax_cap=cap)
            legs["overlap_add"] = lambda: es.render_overlap_add(values, hop, windowed=True)
            es.set_voice_feedback(index)
            for call in legs.values():  # the warm-up: scratch allocations, code objects
                call()
            times = {k: [] for k in legs}
            for _ in range(a.reps):  # legs alternating
                for k, call in legs.items():
                    times[k].append(timed(call))
            es.set_voice_feedback(None)
            es.render_graph_continuous(values, hop)
            plain = [timed(lambda: es.render_graph_continuous(values, hop)) for _ in range(a.reps)]
            best_cap = min(CAPS, key=lambda c: float(np.median(times["relax_%d" % c])))
            wins = all(r < s for r, s in zip(times["relax_%d" % best_cap], times["serial"]))
            row = {"graph": name, "feedback_operator": op, "beta": beta, "no_feedback_graph_continuous": float(np.median(plain)),
                   "best_cap": best_cap, "relax_wins": bool(wins)}
            row.update({k: float(np.median(v)) for k, v in times.items()})
            row["all"] = {k: [round(x, 3) for x in v] for k, v in times.items()}
            result["cases"].append(row)
            print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in row.items() if k != "all"}), flush=True)
        es.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
