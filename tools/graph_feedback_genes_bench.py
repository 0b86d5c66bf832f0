"""What feedback indices as genes (sots_create_graph_genes, the gene form of k_synth_graph) cost, that
nothing else moved, and what the search does with them.

(a) The unchanged path: with no mask, us per generation of the 2-op graph at P = 65536 and of the triple graph at
    P = 32768, N = 1024, through this library and through the parent commit's (--parent-lib), legs alternating over
    --rounds rounds, medians.  Both sides launch the same kernels with the same arguments; expected inside the parent's own
    round-to-round spread.  Both are recorded.
(b) The new form against the fixed-index form: the event-measured time per synthesis launch of the same graphs with the
    same operators feeding back - the carrier(s), and all operators (of the triple graph the first four: a row holds 16
    genes) - once with the index fixed at 1 through the PARENT's
    library (sots_set_voice_feedback) and once as genes whose range is [1, 1], so that every row's gene scales to 1 and
    both legs compute the same audio.  The gene form does per lane what the fixed form does with a scalar operand; the
    expectation is the fixed form's time plus its run-to-run spread.  Ratio and spread are recorded; no threshold.
(c) The search, recorded and not judged: the feedback-sine target of DESIGN.md 4.15, made as tools/graph_feedback_bench.py
    makes it (the additive pair with the second carrier's level 0 and an index of 1 on operator 0 at 430.66 Hz, bin 20 of
    N = 2048, synthesised by the device), eight populations of different seeds (chunks 0 to 7 of one batch, P = 16 + 16),
    one survivor, 1000 generations - the 2-op graph with the carrier's index as a gene, fixed at 1 and fixed at 0, the legs
    "carrier_1" and "none" of profiles/r25_graph_feedback.json: best-ever fitness per seed, and the effective index each
    gene run ends on.  And the 64 shipped noisy chunks with the gene.

One driver process; every leg is a child process of its own (one process loads one library) under its own time limit, one at
a time, and the first leg that fails ends the run.

    python tools/graph_feedback_genes_bench.py --parent-lib /path/to/parent/libsots_hip.so --out profiles/r28_graph_feedback_genes.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from track_overhead import load_pkg, targets  # noqa: E402

PMAX_2OP = [3520.0, 8.0, 3520.0, 1.0]
# name: ((operators, modulators, carriers), param_max of the 2 OPS genes)
GRAPHS = {
    "graph_2op": ((2, [0, 0b1], 0b10), PMAX_2OP),
    "graph_triple": ((6, [0, 0b1, 0, 0b100, 0, 0b10000], 0b101010), PMAX_2OP * 3),
}
ADDITIVE = (2, [0, 0], 0b11)
UNCHANGED = [("graph_2op", 65536, 1000), ("graph_triple", 32768, 500)]
FORMS = [("graph_2op", 65536), ("graph_triple", 32768)]
LEG_SECONDS = 420


def mask_list(ops, mask):
    return [j for j in range(ops) if mask >> j & 1]


def settle(es, seconds):
    t_end = time.perf_counter() + seconds  # clocks settle under the workload itself
    while time.perf_counter() < t_end:
        es.execute_generations(100)
        es.synchronize()


def time_leg(args):
    pkg = load_pkg(args.old_abi)
    graph, pmax = GRAPHS[args.voice]
    ops = graph[0]
    kw = dict(audio_log2=10, workgroup_size=32, synth_kind=pkg.capi.SYNTH_GRAPH, graph=pkg.capi.make_voice_graph(*graph))
    if args.genes:  # every gene's range is [index, index]: each row's gene scales to the index
        e = bin(args.genes).count("1")
        es = pkg.HipES(args.p // 4, args.p - args.p // 4, param_min=[0.0] * (2 * ops) + [args.index] * e, param_max=pmax + [args.index] * e,
                       feedback_genes=args.genes, **kw)
    else:
        es = pkg.HipES(args.p // 4, args.p - args.p // 4, param_max=pmax, **kw)
        if args.fixed:
            es.set_voice_feedback([args.index if args.fixed >> j & 1 else 0.0 for j in range(ops)])
    es.set_target_audio(targets(1, 1024)[0])
    es.init_population(0)
    settle(es, args.settle)
    reps = []
    for _ in range(args.reps):
        es.init_population(0)
        es.synchronize()
        t0 = time.perf_counter()
        es.execute_generations(args.gens)
        es.synchronize()
        reps.append((time.perf_counter() - t0) / args.gens * 1e6)
    es.timing_enable(True)
    es.timing_reset()
    es.execute_generations(min(args.gens, 200))
    es.synchronize()
    ms, count = es.stage_time_ms(pkg.capi.STAGE_FUSED_SYNTH)
    es.close()
    print(json.dumps(dict(voice=args.voice, genes=args.genes, fixed=args.fixed, index=args.index, p=args.p, gens=args.gens,
                          us_per_generation=round(statistics.median(reps), 3), reps=[round(r, 3) for r in reps],
                          synth_us_per_launch=round(ms * 1e3 / count, 3) if count else None)))


def feedback_sine_target(pkg, log2n):
    """DESIGN.md 4.15's target, as tools/graph_feedback_bench.py's rich_target makes it: the additive pair, the second
    carrier's level 0, an index of 1 on operator 0 at bin 20 of N = 2048 - one feedback sine"""
    es = pkg.HipES(32, 32, audio_log2=log2n, workgroup_size=32, synth_kind=pkg.capi.SYNTH_GRAPH, param_max=[430.6640625, 1.0, 430.6640625, 0.0],
                   graph=pkg.capi.make_voice_graph(*ADDITIVE), feedback=[1.0, 0.0])
    es.write_population(values=np.ones((64, 4), np.float32))
    es.synthesise()
    audio = es.read_audio()[0].copy()
    es.close()
    return audio


def search_leg(args):
    pkg = load_pkg(False)
    log2n = 11
    chunks = 64 if args.shipped else 8
    graph, pmax = GRAPHS["graph_2op"]
    tg = targets(chunks, 1 << log2n) if args.shipped else np.tile(feedback_sine_target(pkg, log2n), (chunks, 1))
    kw = dict(audio_log2=log2n, workgroup_size=32, synth_kind=pkg.capi.SYNTH_GRAPH, graph=pkg.capi.make_voice_graph(*graph))
    if args.genes:
        b = pkg.HipBatch(chunks, 16, 16, param_max=pmax + [2.0], feedback_genes=args.genes, **kw)
    else:
        b = pkg.HipBatch(chunks, 16, 16, param_max=pmax, feedback=[0.0, args.index], **kw)
    b.track()
    b.set_survivors(1)
    b.set_target_audio(tg)
    b.init_population(0)
    b.execute_generations(args.gens)
    b.synchronize()
    values, _, ever, _ = b.best_ever()
    b.close()
    out = dict(leg="gene" if args.genes else f"fixed_{args.index:g}", target="shipped" if args.shipped else "feedback_sine", chunks=chunks,
               gens=args.gens, survivors=1, best_ever=[float(x) for x in ever], best_ever_mean=float(np.mean(ever, dtype=np.float64)),
               best_ever_median=float(np.median(ever)))
    if args.genes:
        p = np.float32(0.0) + values[:, 4] * np.float32(2.0)
        out["ends_on_index"] = [float(x) for x in np.where(p > 0, np.minimum(p, np.float32(2.0)), np.float32(0.0))]
    print(json.dumps(out))


def child(extra, lib=None):
    env = dict(os.environ)
    if lib:
        env["SOTS_LIB_PATH"] = lib
    else:
        env.pop("SOTS_LIB_PATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, env=env, capture_output=True, text=True, timeout=LEG_SECONDS)
    if out.returncode != 0:  # (nothing more is started on the device after a leg that failed)
        raise SystemExit(f"leg {extra} failed with {out.returncode}:\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["time", "search"])
    ap.add_argument("--voice", choices=sorted(GRAPHS), default="graph_2op")
    ap.add_argument("--genes", type=int, default=0, help="mask of the operators whose index is a gene")
    ap.add_argument("--fixed", type=int, default=0, help="mask of the operators whose index is fixed at --index")
    ap.add_argument("--index", type=float, default=1.0)
    ap.add_argument("--shipped", action="store_true", help="search leg: the 64 shipped noisy chunks instead of the feedback-sine target")
    ap.add_argument("--p", type=int, default=65536)
    ap.add_argument("--gens", type=int, default=1000)
    ap.add_argument("--old-abi", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of the workload before the timed repetitions")
    ap.add_argument("--parent-lib", help="libsots_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", default="abc", help="which of (a), (b), (c) to run")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.leg == "time":
        return time_leg(args)
    if args.leg == "search":
        return search_leg(args)

    def timed(voice, p, gens, genes=0, fixed=0, lib=None, old=False, reps=args.reps):
        extra = ["--leg", "time", "--voice", voice, "--p", str(p), "--gens", str(gens), "--reps", str(reps), "--settle", str(args.settle),
                 "--genes", str(genes), "--fixed", str(fixed)]
        return child(extra + (["--old-abi"] if old else []), lib)

    result = {"what": __doc__.split("\n\n")[1:4]}
    if "a" in args.parts:
        result["a_unchanged_path"] = []
        for voice, p, gens in UNCHANGED:
            legs = {"new": dict()}
            if args.parent_lib:
                legs["parent"] = dict(lib=args.parent_lib, old=True)
            r = {"voice": voice, "p": p, "gens": gens, **{k: [] for k in legs}}
            for k in range(args.rounds):
                for name in (list(legs) if k % 2 == 0 else list(legs)[::-1]):  # no leg always runs last
                    r[name].append(timed(voice, p, gens, **legs[name])["us_per_generation"])
            for name in legs:
                r[name + "_median"] = statistics.median(r[name])
            if args.parent_lib:
                r["parent_spread"] = round(max(r["parent"]) - min(r["parent"]), 3)
                r["new_spread"] = round(max(r["new"]) - min(r["new"]), 3)
                r["inside_the_parents_spread"] = bool(r["new_median"] <= r["parent_median"] + r["parent_spread"])
            else:
                r["inside_the_parents_spread"] = "not yet taken (no --parent-lib)"
            result["a_unchanged_path"].append(r)
            print(json.dumps(r), flush=True)
    if "b" in args.parts:
        result["b_gene_form_against_fixed_form"] = []
        fixed_lib = dict(lib=args.parent_lib, old=True) if args.parent_lib else dict()
        for voice, p in FORMS:
            ops, _, carriers = GRAPHS[voice][0]
            fit = min(ops, 16 - 2 * ops)  # (a row holds 16 genes: the triple graph has room for four indices)
            for who, mask in (("carriers", carriers), ("all" if fit == ops else f"the first {fit}", (1 << fit) - 1)):
                legs = {"fixed": dict(fixed=mask, **fixed_lib), "genes": dict(genes=mask)}
                r = {"voice": voice, "p": p, "operators_feeding_back": mask_list(ops, mask), "which": who, "index": 1.0,
                     "fixed_form_through": "the parent's library" if args.parent_lib else "this library (no --parent-lib)",
                     "rounds": {k: [] for k in legs}}
                for k in range(args.rounds):
                    for name in (list(legs) if k % 2 == 0 else list(legs)[::-1]):
                        r["rounds"][name].append(timed(voice, p, 200, reps=2, **legs[name])["synth_us_per_launch"])
                m = {name: statistics.median(r["rounds"][name]) for name in legs}
                r["synth_us_per_launch"] = m
                r["fixed_spread_us"] = round(max(r["rounds"]["fixed"]) - min(r["rounds"]["fixed"]), 3)
                r["genes_over_fixed"] = round(m["genes"] / m["fixed"], 4)
                r["genes_minus_fixed_us"] = round(m["genes"] - m["fixed"], 3)
                r["inside_fixed_plus_spread"] = bool(m["genes"] <= m["fixed"] + r["fixed_spread_us"])
                result["b_gene_form_against_fixed_form"].append(r)
                print(json.dumps(r), flush=True)
    if "c" in args.parts:
        result["c_the_search"] = []
        for extra in (["--genes", "2"], ["--index", "1"], ["--index", "0"], ["--genes", "2", "--shipped"]):
            q = child(["--leg", "search", "--gens", "1000"] + extra)
            result["c_the_search"].append(q)
            print(json.dumps(q), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
