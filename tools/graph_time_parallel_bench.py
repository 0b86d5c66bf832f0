"""What the graph voice's time-parallel synthesis form (k_synth_graph_tp, sots_set_graph_synth_form) costs
beside the lane form, and where AUTO may take it.

(a) Graphs 2op, chain3, two_mods, fan3 and triple at N = 1024 and 2048, populations of 32, 1024, 2048, 3072 and 4096 rows
    (a CU's share of 1, 4, 8, 12 and 16 on 256 CUs) as far as they fit one group per workgroup, and the largest that does
    (capacity x CUs).  One context per case; the LANES and TIME_PARALLEL legs alternate over --rounds rounds in this one
    process (the form is a setting of the context).  A leg is --gens generations of the fused loop: us per generation from the
    wall clock around execute_generations + synchronise, then the event-timed synthesis launch (sots_stage_time_ms).  Medians
    over the rounds and each leg's round-to-round spread (max - min).  The LANES leg is the yardstick: the kernel and the
    arguments the library launched before there were forms.
(b) The fixed voices 2op and triple_parallel, which run k_synth_tp at these sizes, at the same populations: how far the graph
    form is from a hand-specialised one.
(c) The shipped shape, 64 chunks x (16 + 16) in flight at N = 2048 (2048 rows per launch), on 2op, additive and chain3: us
    per generation of sots_batch_execute_generations under both forms.
(d) Per operator count, the largest share up to which TIME_PARALLEL beat LANES, in synthesis launch time AND per generation,
    in every round by more than the LANES leg's own spread, at both N and at every measured share below it: what
    kGraphTpAutoShare (csrc/sots_rules.h) may hold.

    python tools/graph_time_parallel_bench.py --out profiles/r33_graph_time_parallel.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from track_overhead import load_pkg, targets  # noqa: E402

PMAX_2OP = [3520.0, 8.0, 3520.0, 1.0]
CHAIN = [3520.0, 8.0, 3520.0, 8.0, 3520.0, 1.0]
GRAPHS = {
    "2op": ((2, [0, 0b1], 0b10), PMAX_2OP),
    "chain3": ((3, [0, 0b1, 0b10], 0b100), CHAIN),
    "two_mods": ((3, [0, 0, 0b011], 0b100), CHAIN),
    "fan3": ((4, [0, 0, 0, 0b0111], 0b1000), [3520.0, 8.0] * 3 + [3520.0, 1.0]),
    "triple": ((6, [0, 0b1, 0, 0b100, 0, 0b10000], 0b101010), PMAX_2OP * 3),
    "additive": ((2, [0, 0], 0b11), [3520.0, 1.0, 3520.0, 1.0]),
}
FIXED = {"2op": (0, PMAX_2OP), "triple": (2, PMAX_2OP + [0.0] * 8)}
LANES, TIME = 1, 2
FORMS = {"lanes": LANES, "time_parallel": TIME}


def timed(pkg, handle, gens, reps, context=True):
    """(us per generation, us per synthesis launch or None): medians of `reps` repetitions"""
    per_gen = []
    for _ in range(reps):
        handle.init_population(0)
        handle.synchronize()
        t0 = time.perf_counter()
        handle.execute_generations(gens)
        handle.synchronize()
        per_gen.append((time.perf_counter() - t0) / gens * 1e6)
    synth = None
    if context:
        handle.timing_enable(True)
        handle.timing_reset()
        handle.execute_generations(gens)
        handle.synchronize()
        ms, count = handle.stage_time_ms(pkg.capi.STAGE_FUSED_SYNTH)
        synth = ms * 1e3 / count if count else None
        handle.timing_enable(False)
    return statistics.median(per_gen), synth


def summary(rounds):
    out = {}
    for leg, rows in rounds.items():
        for key in ("us_per_generation", "synth_us_per_launch"):
            xs = [r[key] for r in rows if r[key] is not None]
            if xs:
                out[f"{leg}_{key}"] = round(statistics.median(xs), 3)
                out[f"{leg}_{key}_spread"] = round(max(xs) - min(xs), 3)
    return out


def time_wins(rounds, key):
    """TIME_PARALLEL below LANES in every round by more than the LANES leg's round-to-round spread"""
    lanes = [r[key] for r in rounds["lanes"]]
    tp = [r[key] for r in rounds["time_parallel"]]
    spread = max(lanes) - min(lanes)
    return all(t < l - spread for t, l in zip(tp, lanes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gens", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--settle", type=float, default=0.5, help="seconds of the workload before a case's first round")
    ap.add_argument("--out")
    args = ap.parse_args()
    pkg = load_pkg(False)
    hip = pkg.capi
    result = {"what": __doc__.split("\n\n")[1:5], "a_forms": [], "b_fixed_voices": [], "c_shipped_shape": [], "d_auto_share": {}}

    def settle(handle):
        t_end = time.perf_counter() + args.settle
        while time.perf_counter() < t_end:
            handle.execute_generations(100)
            handle.synchronize()

    cus = None
    for name in ("2op", "chain3", "two_mods", "fan3", "triple"):
        graph, pmax = GRAPHS[name]
        cap, levels = hip.graph_time_parallel_capacity(hip.make_voice_graph(*graph))
        for log2n in (10, 11):
            for p in sorted({32, 1024, 2048, 3072, 4096, cap * (cus or 256)}):
                if cus is not None and p > cap * cus:
                    continue
                es = pkg.HipES(p // 4, p - p // 4, synth_kind=hip.SYNTH_GRAPH, audio_log2=log2n, param_max=pmax, workgroup_size=8,
                               graph=hip.make_voice_graph(*graph))
                cus = es.info().compute_units
                if p > cap * cus:
                    es.close()
                    continue
                es.set_target_audio(targets(1, 1 << log2n)[0])
                es.init_population(0)
                settle(es)
                rounds = {leg: [] for leg in FORMS}
                for k in range(args.rounds):
                    for leg in (list(FORMS) if k % 2 == 0 else list(FORMS)[::-1]):  # neither form always runs second
                        es.set_graph_synth_form(FORMS[leg])
                        assert es.graph_synth_form() == (FORMS[leg], FORMS[leg])
                        us, synth = timed(pkg, es, args.gens, args.reps)
                        rounds[leg].append({"us_per_generation": round(us, 3), "synth_us_per_launch": round(synth, 3)})
                es.close()
                share = (p + cus - 1) // cus
                r = dict(graph=name, operators=graph[0], levels=levels, capacity=cap, n=1 << log2n, p=p, share=share, compute_units=cus,
                         **summary(rounds), time_parallel_wins_synth=time_wins(rounds, "synth_us_per_launch"),
                         time_parallel_wins_generation=time_wins(rounds, "us_per_generation"), rounds=rounds)
                result["a_forms"].append(r)
                print(json.dumps({k: v for k, v in r.items() if k != "rounds"}), flush=True)
                # (b) the fixed voice that this graph restates, where k_synth_tp takes the share
                if name in FIXED:
                    kind, fmax = FIXED[name]
                    fx = pkg.HipES(p // 4, p - p // 4, synth_kind=kind, audio_log2=log2n, param_max=fmax, workgroup_size=8)
                    fx.set_target_audio(targets(1, 1 << log2n)[0])
                    fx.init_population(0)
                    settle(fx)
                    rows = []
                    for _ in range(args.rounds):
                        us, synth = timed(pkg, fx, args.gens, args.reps)
                        rows.append({"us_per_generation": round(us, 3), "synth_us_per_launch": round(synth, 3)})
                    fx.close()
                    f = dict(voice=name, n=1 << log2n, p=p, share=share, **summary({"fixed": rows}), rounds=rows)
                    result["b_fixed_voices"].append(f)
                    print(json.dumps({k: v for k, v in f.items() if k != "rounds"}), flush=True)
    # (c) the shipped shape
    for name in ("2op", "additive", "chain3"):
        graph, pmax = GRAPHS[name]
        b = pkg.HipBatch(64, 16, 16, synth_kind=hip.SYNTH_GRAPH, audio_log2=11, param_max=pmax, workgroup_size=16,
                         graph=hip.make_voice_graph(*graph))
        b.set_survivors(1)
        b.set_target_audio(targets(64, 2048))
        b.init_population(0)
        settle(b)
        rounds = {leg: [] for leg in FORMS}
        for k in range(args.rounds):
            for leg in (list(FORMS) if k % 2 == 0 else list(FORMS)[::-1]):
                b.set_graph_synth_form(FORMS[leg])
                assert b.graph_synth_form() == (FORMS[leg], FORMS[leg])
                us, _ = timed(pkg, b, args.gens, args.reps, context=False)
                rounds[leg].append({"us_per_generation": round(us, 3), "synth_us_per_launch": None})
        b.close()
        r = dict(graph=name, chunks=64, p=32, n=2048, rows_per_launch=2048, **summary(rounds),
                 time_parallel_wins_generation=time_wins(rounds, "us_per_generation"), rounds=rounds)
        result["c_shipped_shape"].append(r)
        print(json.dumps({k: v for k, v in r.items() if k != "rounds"}), flush=True)
    # (d) the share up to which the form won everywhere it was measured, per operator count
    for ops in sorted({r["operators"] for r in result["a_forms"]}):
        rows = [r for r in result["a_forms"] if r["operators"] == ops]
        limit = 0
        for share in sorted({r["share"] for r in rows}):
            if all(r["time_parallel_wins_synth"] and r["time_parallel_wins_generation"] for r in rows if r["share"] == share):
                limit = share
            else:
                break
        result["d_auto_share"][str(ops)] = limit
    print(json.dumps(result["d_auto_share"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
