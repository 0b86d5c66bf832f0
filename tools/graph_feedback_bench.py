"""What the graph voice's per-operator feedback (sots_set_voice_feedback, the feedback form of k_synth_graph) costs, that
nothing else moved, and what it is for.

(a) Nothing moved: us per generation of the 2-op graph at BASELINE configs[2] (P = 16384 + 49152, N = 1024) and of the triple
    graph at P = 32768 - with no setting, with all-zero set, and through the parent commit's library (--parent-lib) - legs
    alternating over --rounds rounds, medians.  Accepted when the new median is no higher than the parent's median plus the
    parent's own round-to-round spread: both sides launch the same kernel.
(b) What feedback costs: the event-measured time per synthesis launch of the 2-op graph at P = 65536 and of the six-operator
    triple graph at P = 32768, N = 1024, with an index of 1 on one operator (operator 0) and on all, beside the all-sine
    launch of the same graph, the all-sine launch of that graph with one more operator (a second modulator into carrier 1)
    and the launch with one SAW operator (operator 0).  The claim under test: a feedback operator costs less than an added
    operator.  Recorded as held or refuted.
(c) What it is for, recorded and not judged: the 64 shipped noisy chunks (N = 2048, P = 16 + 16), 64 in flight, 1000
    generations, one survivor - best-ever mean and median of the 2-op graph with an index of 0, 0.5 and 1 on the modulator
    and on the carrier; and the same legs against ONE harmonic-rich target, eight populations of different seeds: the
    additive pair with the second carrier's level 0 and an index of 1 on operator 0 at 430.66 Hz, synthesised by the
    device (tests/test_gpu_graph_feedback.py holds the device to the model, tests/test_graph_feedback_cpu.py the host's
    synthesiser to the same model, bit for bit).

Every leg is a child process (one process loads one library).

    python tools/graph_feedback_bench.py --parent-lib /path/to/parent/libsots_hip.so --out profiles/r25_graph_feedback.json
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
# name: ((operators, modulators, carriers), param_max)
# "plus one": the same graph with a second modulator into its first carrier
GRAPHS = {
    "graph_2op": ((2, [0, 0b1], 0b10), PMAX_2OP),
    "graph_2op_plus_one": ((3, [0, 0, 0b011], 0b100), [3520.0, 8.0] + PMAX_2OP),
    "graph_triple": ((6, [0, 0b1, 0, 0b100, 0, 0b10000], 0b101010), PMAX_2OP * 3),
    "graph_triple_plus_one": ((7, [0, 0, 0b11, 0, 0b1000, 0, 0b100000], 0b1010100), [3520.0, 8.0] + PMAX_2OP * 3),
}
ADDITIVE = (2, [0, 0], 0b11)
NOTHING_MOVED = [("graph_2op", 65536, 1000), ("graph_triple", 32768, 500)]
COSTS = [("graph_2op", "graph_2op_plus_one", 65536), ("graph_triple", "graph_triple_plus_one", 32768)]
QUALITY = {"none": None, "modulator_0.5": [0.5, 0.0], "modulator_1": [1.0, 0.0], "carrier_0.5": [0.0, 0.5], "carrier_1": [0.0, 1.0]}
SAW = 7


def settle(es, seconds):
    t_end = time.perf_counter() + seconds  # clocks settle under the workload itself
    while time.perf_counter() < t_end:
        es.execute_generations(100)
        es.synchronize()


def time_leg(args):
    pkg = load_pkg(args.old_abi)
    graph, pmax = GRAPHS[args.voice]
    es = pkg.HipES(args.p // 4, args.p - args.p // 4, audio_log2=10, workgroup_size=32, synth_kind=pkg.capi.SYNTH_GRAPH, param_max=pmax,
                   graph=pkg.capi.make_voice_graph(*graph))
    if args.waves is not None:
        es.set_voice_waveforms(json.loads(args.waves))
    if args.feedback is not None:
        es.set_voice_feedback(json.loads(args.feedback))
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
    print(json.dumps(dict(voice=args.voice, waves=args.waves, feedback=args.feedback, p=args.p, gens=args.gens,
                          us_per_generation=round(statistics.median(reps), 3), reps=[round(r, 3) for r in reps],
                          synth_us_per_launch=round(ms * 1e3 / count, 3) if count else None)))


def rich_target(pkg, log2n):
    """the additive pair, the second carrier's level 0, an index of 1 on operator 0 at bin 20 of N = 2048"""
    es = pkg.HipES(32, 32, audio_log2=log2n, workgroup_size=32, synth_kind=pkg.capi.SYNTH_GRAPH, param_max=[430.6640625, 1.0, 430.6640625, 0.0],
                   graph=pkg.capi.make_voice_graph(*ADDITIVE), feedback=[1.0, 0.0])
    es.write_population(values=np.ones((64, 4), np.float32))
    es.synthesise()
    row = es.read_audio()[0].copy()
    es.close()
    return row


def quality_leg(args):
    pkg = load_pkg(False)
    log2n = 11
    chunks = 8 if args.rich else 64
    graph, pmax = GRAPHS["graph_2op"]
    tg = np.tile(rich_target(pkg, log2n), (chunks, 1)) if args.rich else targets(chunks, 1 << log2n)
    b = pkg.HipBatch(chunks, 16, 16, audio_log2=log2n, workgroup_size=32, synth_kind=pkg.capi.SYNTH_GRAPH, param_max=pmax,
                     graph=pkg.capi.make_voice_graph(*graph), feedback=None if args.feedback is None else json.loads(args.feedback))
    b.track()
    b.set_survivors(1)
    b.set_target_audio(tg)
    b.init_population(0)
    b.execute_generations(args.gens)
    b.synchronize()
    ever = b.best_ever()[2].astype(np.float64)
    b.close()
    print(json.dumps(dict(feedback=args.feedback, target="rich" if args.rich else "shipped", chunks=chunks, gens=args.gens, survivors=1,
                          best_ever_mean=float(ever.mean()), best_ever_median=float(np.median(ever)), best_ever_min=float(ever.min()))))


def child(extra, lib=None):
    env = dict(os.environ)
    if lib:
        env["SOTS_LIB_PATH"] = lib
    else:
        env.pop("SOTS_LIB_PATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"leg {extra} failed:\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["time", "quality"])
    ap.add_argument("--voice", choices=sorted(GRAPHS), default="graph_2op")
    ap.add_argument("--waves", help="JSON list of codes, one per operator; absent: no setting")
    ap.add_argument("--feedback", help="JSON list of indices, one per operator; absent: no setting")
    ap.add_argument("--rich", action="store_true", help="quality leg: the harmonic-rich target instead of the shipped chunks")
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
    if args.leg == "quality":
        return quality_leg(args)

    def timed(voice, p, gens, waves=None, feedback=None, lib=None, old=False, reps=args.reps):
        extra = ["--leg", "time", "--voice", voice, "--p", str(p), "--gens", str(gens), "--reps", str(reps), "--settle", str(args.settle)]
        if waves is not None:
            extra += ["--waves", json.dumps(waves)]
        if feedback is not None:
            extra += ["--feedback", json.dumps(feedback)]
        return child(extra + (["--old-abi"] if old else []), lib)

    result = {"what": __doc__.split("\n\n")[1:4]}
    if "a" in args.parts:
        result["a_nothing_moved"] = []
        for voice, p, gens in NOTHING_MOVED:
            ops = GRAPHS[voice][0][0]
            legs = {"no_setting": dict(), "all_zero_set": dict(feedback=[0.0] * ops)}
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
                r["accepted"] = bool(max(r["no_setting_median"], r["all_zero_set_median"]) <= r["parent_median"] + r["parent_spread"])
            else:
                r["accepted"] = "not yet taken (no --parent-lib)"
            result["a_nothing_moved"].append(r)
            print(json.dumps(r), flush=True)
    if "b" in args.parts:
        result["b_what_feedback_costs"] = []
        for voice, plus_one, p in COSTS:
            ops = GRAPHS[voice][0][0]
            one = [1.0] + [0.0] * (ops - 1)
            legs = {"sine": dict(voice=voice), "sine_one_more_operator": dict(voice=plus_one),
                    "saw_on_one": dict(voice=voice, waves=[SAW] + [0] * (ops - 1)),
                    "feedback_on_one": dict(voice=voice, feedback=one), "feedback_on_all": dict(voice=voice, feedback=[1.0] * ops)}
            r = {"voice": voice, "one_more_operator": plus_one, "p": p, "index": 1.0, "rounds": {k: [] for k in legs}}
            for k in range(args.rounds):
                for name in (list(legs) if k % 2 == 0 else list(legs)[::-1]):
                    r["rounds"][name].append(timed(p=p, gens=200, reps=2, **legs[name])["synth_us_per_launch"])
            r["synth_us_per_launch"] = {name: statistics.median(r["rounds"][name]) for name in legs}
            m = r["synth_us_per_launch"]
            r["an_operator_costs_us"] = round(m["sine_one_more_operator"] - m["sine"], 3)
            r["one_feedback_operator_costs_us"] = round(m["feedback_on_one"] - m["sine"], 3)
            r["feedback_on_all_costs_us_per_operator"] = round((m["feedback_on_all"] - m["sine"]) / ops, 3)
            r["one_saw_operator_costs_us"] = round(m["saw_on_one"] - m["sine"], 3)
            r["a_feedback_operator_costs_less_than_an_operator"] = "held" if r["one_feedback_operator_costs_us"] < r["an_operator_costs_us"] else "refuted"
            r["per_operator_with_all_fed_back_costs_less_than_an_operator"] = (
                "held" if r["feedback_on_all_costs_us_per_operator"] < r["an_operator_costs_us"] else "refuted")
            result["b_what_feedback_costs"].append(r)
            print(json.dumps({k: v for k, v in r.items() if k != "rounds"}), flush=True)
    if "c" in args.parts:
        result["c_what_it_is_for"] = []
        for rich in (False, True):
            for name, feedback in QUALITY.items():
                extra = ["--leg", "quality", "--gens", "1000"] + (["--rich"] if rich else [])
                q = child(extra + ([] if feedback is None else ["--feedback", json.dumps(feedback)]))
                q["setting"] = name
                result["c_what_it_is_for"].append(q)
                print(json.dumps(q), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
