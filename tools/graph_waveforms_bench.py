"""What the graph voice's operator waveforms (sots_set_voice_waveforms, the shaped form of k_synth_graph) cost, that
nothing else moved, and what they are for.

(a) Nothing moved: us per generation of the 2-op graph at BASELINE configs[2] (P = 16384 + 49152, N = 1024) and of the triple
    graph at P = 32768 - with no setting, with all-sine set, and through the parent commit's library (--parent-lib) - legs
    alternating over --rounds rounds, medians.  Accepted when the new median is no higher than the parent's median plus the
    parent's own round-to-round spread.
(b) What a shape costs: the event-measured time per synthesis launch of the 2-op graph and of the six-operator triple graph
    with one code on every operator (each of the seven) and with mixed codes, beside the sine launch of the same graph and
    the sine launch of that graph with one more operator (a second modulator into carrier 1).  The claim to confirm or
    refute: a shape costs less than an operator.  With --exp-lib (this tree's library built with EXTRA=-DSOTS_EXPERIMENT)
    the mixed, the HALF and the SAW legs also run as the form that was not kept: one branchless body with per-operator scalar
    constants (SOTS_GRAPH_SHAPE_CONSTANTS=1).
(c) What it is for, recorded and not judged: the 64 shipped noisy chunks (N = 2048, P = 16 + 16), 64 in flight, 1000
    generations, one survivor - best-ever mean and median of the 2-op graph all sine, with a HALF modulator, with a HALF
    carrier and with a SAW modulator.

Every leg is a child process (one process loads one library).

    python tools/graph_waveforms_bench.py --parent-lib /path/to/parent/libsots_hip.so --out profiles/r24_graph_waveforms.json
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
NOTHING_MOVED = [("graph_2op", 65536, 1000), ("graph_triple", 32768, 500)]
COSTS = [("graph_2op", "graph_2op_plus_one", 65536), ("graph_triple", "graph_triple_plus_one", 32768)]
NAMES = ["sine", "half", "abs", "pulse", "even", "absEven", "square", "saw"]
QUALITY = {"sine": None, "half_modulator": [1, 0], "half_carrier": [0, 1], "saw_modulator": [7, 0]}


def mixed(ops):
    return [(j + 1) % 8 for j in range(ops)]


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
    print(json.dumps(dict(voice=args.voice, waves=args.waves, p=args.p, gens=args.gens, us_per_generation=round(statistics.median(reps), 3),
                          reps=[round(r, 3) for r in reps], synth_us_per_launch=round(ms * 1e3 / count, 3) if count else None)))


def quality_leg(args):
    pkg = load_pkg(False)
    chunks, log2n = 64, 11
    graph, pmax = GRAPHS["graph_2op"]
    b = pkg.HipBatch(chunks, 16, 16, audio_log2=log2n, workgroup_size=32, synth_kind=pkg.capi.SYNTH_GRAPH, param_max=pmax,
                     graph=pkg.capi.make_voice_graph(*graph), waveforms=None if args.waves is None else json.loads(args.waves))
    b.track()
    b.set_survivors(1)
    b.set_target_audio(targets(chunks, 1 << log2n))
    b.init_population(0)
    b.execute_generations(args.gens)
    b.synchronize()
    ever = b.best_ever()[2].astype(np.float64)
    b.close()
    print(json.dumps(dict(waves=args.waves, chunks=chunks, gens=args.gens, survivors=1, best_ever_mean=float(ever.mean()),
                          best_ever_median=float(np.median(ever)))))


def child(extra, lib=None, env_extra=None):
    env = dict(os.environ)
    if lib:
        env["SOTS_LIB_PATH"] = lib
    else:
        env.pop("SOTS_LIB_PATH", None)
    env.update(env_extra or {})
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, env=env, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"leg {extra} failed:\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["time", "quality"])
    ap.add_argument("--voice", choices=sorted(GRAPHS), default="graph_2op")
    ap.add_argument("--waves", help="JSON list of codes, one per operator; absent: no setting")
    ap.add_argument("--p", type=int, default=65536)
    ap.add_argument("--gens", type=int, default=1000)
    ap.add_argument("--old-abi", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of the workload before the timed repetitions")
    ap.add_argument("--parent-lib", help="libsots_hip.so built from the parent commit")
    ap.add_argument("--exp-lib", help="this tree's libsots_hip.so built with EXTRA=-DSOTS_EXPERIMENT")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", default="abc", help="which of (a), (b), (c) to run")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.leg == "time":
        return time_leg(args)
    if args.leg == "quality":
        return quality_leg(args)

    def timed(voice, p, gens, waves=None, lib=None, env=None, old=False, reps=args.reps):
        extra = ["--leg", "time", "--voice", voice, "--p", str(p), "--gens", str(gens), "--reps", str(reps), "--settle", str(args.settle)]
        if waves is not None:
            extra += ["--waves", json.dumps(waves)]
        return child(extra + (["--old-abi"] if old else []), lib, env)

    result = {"what": __doc__.split("\n\n")[1:4]}
    if "a" in args.parts:
        result["a_nothing_moved"] = []
        for voice, p, gens in NOTHING_MOVED:
            ops = GRAPHS[voice][0][0]
            legs = {"no_setting": dict(), "all_sine_set": dict(waves=[0] * ops)}
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
                r["accepted"] = bool(max(r["no_setting_median"], r["all_sine_set_median"]) <= r["parent_median"] + r["parent_spread"])
            else:
                r["accepted"] = "not yet taken (no --parent-lib)"
            result["a_nothing_moved"].append(r)
            print(json.dumps(r), flush=True)
    if "b" in args.parts:
        result["b_what_a_shape_costs"] = []
        for voice, plus_one, p in COSTS:
            ops = GRAPHS[voice][0][0]
            legs = {"sine": dict(voice=voice), "sine_one_more_operator": dict(voice=plus_one), "mixed": dict(voice=voice, waves=mixed(ops))}
            for w in range(1, 8):
                legs[NAMES[w]] = dict(voice=voice, waves=[w] * ops)
            if args.exp_lib:
                env = {"SOTS_GRAPH_SHAPE_CONSTANTS": "1"}
                legs["mixed_constants"] = dict(voice=voice, waves=mixed(ops), lib=args.exp_lib, env=env)
                legs["saw_constants"] = dict(voice=voice, waves=[7] * ops, lib=args.exp_lib, env=env)
                legs["half_constants"] = dict(voice=voice, waves=[1] * ops, lib=args.exp_lib, env=env)
            r = {"voice": voice, "one_more_operator": plus_one, "p": p, "mixed_codes": mixed(ops), "rounds": {k: [] for k in legs}}
            for k in range(args.rounds):
                for name in (list(legs) if k % 2 == 0 else list(legs)[::-1]):
                    r["rounds"][name].append(timed(p=p, gens=200, reps=2, **legs[name])["synth_us_per_launch"])
            r["synth_us_per_launch"] = {name: statistics.median(r["rounds"][name]) for name in legs}
            m = r["synth_us_per_launch"]
            r["an_operator_costs_us"] = round(m["sine_one_more_operator"] - m["sine"], 3)
            r["the_dearest_shape_costs_us"] = round(max(m[n] for n in NAMES[1:] + ["mixed"]) - m["sine"], 3)
            r["a_shape_costs_less_than_an_operator"] = bool(r["the_dearest_shape_costs_us"] < r["an_operator_costs_us"])
            result["b_what_a_shape_costs"].append(r)
            print(json.dumps({k: v for k, v in r.items() if k != "rounds"}), flush=True)
    if "c" in args.parts:
        result["c_64_shipped_chunks"] = []
        for name, waves in QUALITY.items():
            q = child(["--leg", "quality", "--gens", "1000"] + ([] if waves is None else ["--waves", json.dumps(waves)]))
            q["setting"] = name
            result["c_64_shipped_chunks"].append(q)
            print(json.dumps(q), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
