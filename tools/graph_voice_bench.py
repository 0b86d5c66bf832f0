"""What the operator-graph voice (SOTS_SYNTH_GRAPH, k_synth_graph) costs beside the fixed voices it can restate, that the
fixed voices cost what they did, and what the voice is for.

(a) The anchor graphs against the fixed voices they equal bit for bit, one context each: the 2-op voice and its graph at
    BASELINE configs[2] (P = 16384 + 49152, N = 1024) and at P = 1024, the triple voice and its graph at P = 32768 and at
    P = 1024.  us per generation = wall time of execute_generations(G) + synchronise, / G, median of --reps repetitions
    after --settle seconds of the workload; then, in the same process with the stage timers on, the event-measured time per
    launch of the synthesis stage and of the stand-alone variation launch (0 launches where the synthesis kernel makes its
    individuals itself).  The legs of a comparison alternate over --rounds rounds.  With --exp-lib (this tree's library
    built with EXTRA=-DSOTS_EXPERIMENT) two more legs run through that library: the fixed 2-op voice with
    SOTS_FUSE_VARIATION=0 - the graph voice never fuses, so this is the like-for-like loop - and the graph kernel with
    SOTS_GRAPH_WAVES=8 (two wavefronts per SIMD, half-line tiles) beside the default of one per SIMD.
(b) The fixed voices against the parent commit's library (--parent-lib), alternating, as tools/survivors_bench.py does:
    accepted when the new median is no higher than the parent's median plus the parent's own round-to-round spread.
(c) What the voice is for: the 64 shipped noisy chunks (tests/_survivors_model.py: targets; N = 2048, P = 16 + 16), 64
    chunks in flight, 1000 generations, one survivor, tracked: mean and median best-ever fitness for the 2-op voice, the
    triple voice, the additive pair, the clean chain of three and two modulators into one carrier.  Recorded, not judged.

Every leg is a child process (one process loads one library).

    python tools/graph_voice_bench.py --parent-lib /path/to/parent/libsots_hip.so --out profiles/r22_graph_voice.json
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
# name: (fixed kind or None, graph (operators, modulators, carriers) or None, param_max)
VOICES = {
    "2op": (0, None, PMAX_2OP),
    "graph_2op": (None, (2, [0, 0b1], 0b10), PMAX_2OP),
    "triple_parallel": (2, None, PMAX_2OP + [0.0] * 8),
    "graph_triple": (None, (6, [0, 0b1, 0, 0b100, 0, 0b10000], 0b101010), PMAX_2OP * 3),
    "graph_additive": (None, (2, [0, 0], 0b11), [3520.0, 1.0, 3520.0, 1.0]),
    "graph_chain3": (None, (3, [0, 0b1, 0b10], 0b100), [3520.0, 8.0, 3520.0, 8.0, 3520.0, 1.0]),
    "graph_two_mods": (None, (3, [0, 0, 0b011], 0b100), [3520.0, 8.0, 3520.0, 8.0, 3520.0, 1.0]),
}
# (a): (fixed voice, its graph, population, generations per repetition)
PAIRS = [("2op", "graph_2op", 65536, 1000), ("triple_parallel", "graph_triple", 32768, 500),
         ("2op", "graph_2op", 1024, 2000), ("triple_parallel", "graph_triple", 1024, 2000)]
QUALITY = ["2op", "triple_parallel", "graph_additive", "graph_chain3", "graph_two_mods"]


def voice_kwargs(pkg, name):
    kind, graph, pmax = VOICES[name]
    if graph is None:
        return dict(synth_kind=kind, param_max=pmax)
    return dict(synth_kind=pkg.capi.SYNTH_GRAPH, param_max=pmax, graph=pkg.capi.make_voice_graph(*graph))


def settle(es, seconds):
    t_end = time.perf_counter() + seconds  # clocks settle under the workload itself
    while time.perf_counter() < t_end:
        es.execute_generations(100)
        es.synchronize()


def time_leg(args):
    pkg = load_pkg(args.old_abi)
    es = pkg.HipES(args.p // 4, args.p - args.p // 4, audio_log2=10, workgroup_size=32, **voice_kwargs(pkg, args.voice))
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
    stages = {}
    for key, stage in (("synth", pkg.capi.STAGE_FUSED_SYNTH), ("variation", pkg.capi.STAGE_FUSED_VARIATION)):
        ms, count = es.stage_time_ms(stage)
        stages[key + "_us_per_launch"] = round(ms * 1e3 / count, 3) if count else None
        stages[key + "_launches"] = int(count)
    es.close()
    print(json.dumps(dict(voice=args.voice, p=args.p, gens=args.gens, us_per_generation=round(statistics.median(reps), 3),
                          reps=[round(r, 3) for r in reps], **stages)))


def quality_leg(args):
    pkg = load_pkg(False)
    chunks, log2n = 64, 11
    b = pkg.HipBatch(chunks, 16, 16, audio_log2=log2n, workgroup_size=32, **voice_kwargs(pkg, args.voice))
    b.track()
    b.set_survivors(1)
    b.set_target_audio(targets(chunks, 1 << log2n))
    b.init_population(0)
    b.synchronize()
    t0 = time.perf_counter()
    b.execute_generations(args.gens)
    b.synchronize()
    us = (time.perf_counter() - t0) / args.gens * 1e6
    ever = b.best_ever()[2].astype(np.float64)
    b.close()
    print(json.dumps(dict(voice=args.voice, chunks=chunks, gens=args.gens, survivors=1, us_per_generation=round(us, 3),
                          best_ever_mean=float(ever.mean()), best_ever_median=float(np.median(ever)))))


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
    ap.add_argument("--voice", choices=sorted(VOICES), default="graph_2op")
    ap.add_argument("--p", type=int, default=65536)
    ap.add_argument("--gens", type=int, default=1000)
    ap.add_argument("--old-abi", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of the workload before the timed repetitions")
    ap.add_argument("--parent-lib", help="libsots_hip.so built from the parent commit")
    ap.add_argument("--exp-lib", help="this tree's libsots_hip.so built with EXTRA=-DSOTS_EXPERIMENT")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.leg == "time":
        return time_leg(args)
    if args.leg == "quality":
        return quality_leg(args)

    common = ["--reps", str(args.reps), "--settle", str(args.settle)]

    def timed(voice, p, gens, lib=None, env=None, old=False):
        return child(["--leg", "time", "--voice", voice, "--p", str(p), "--gens", str(gens)] + common + (["--old-abi"] if old else []), lib, env)

    result = {"what": __doc__.split("\n\n")[1:4], "a_graph_against_fixed": [], "b_fixed_against_parent": [], "c_64_shipped_chunks": []}
    for fixed, graph, p, gens in PAIRS:
        legs = {"fixed": (fixed, None, None), "graph": (graph, None, None)}
        if args.exp_lib and fixed == "2op":
            legs["fixed_unfused"] = (fixed, args.exp_lib, {"SOTS_FUSE_VARIATION": "0"})
        if args.exp_lib:
            legs["graph_8_waves"] = (graph, args.exp_lib, {"SOTS_GRAPH_WAVES": "8"})
        r = {"p": p, "gens": gens, "fixed_voice": fixed, "graph_voice": graph, "rounds": {k: [] for k in legs}}
        for k in range(args.rounds):
            order = list(legs) if k % 2 == 0 else list(legs)[::-1]  # no leg always runs last
            for name in order:
                voice, lib, env = legs[name]
                r["rounds"][name].append(timed(voice, p, gens, lib, env))
        for name in legs:
            r[name + "_us_per_generation"] = statistics.median(x["us_per_generation"] for x in r["rounds"][name])
            synth = [x["synth_us_per_launch"] for x in r["rounds"][name] if x["synth_us_per_launch"] is not None]
            r[name + "_synth_us_per_launch"] = statistics.median(synth) if synth else None
        r["graph_over_fixed_us_per_generation"] = round(r["graph_us_per_generation"] / r["fixed_us_per_generation"], 3)
        if "fixed_unfused" in legs:
            r["graph_over_fixed_unfused_us_per_generation"] = round(r["graph_us_per_generation"] / r["fixed_unfused_us_per_generation"], 3)
        result["a_graph_against_fixed"].append(r)
        print(json.dumps({k: v for k, v in r.items() if k != "rounds"}), flush=True)
    if args.parent_lib:
        for voice, _, p, gens in PAIRS[:2]:
            r = {"voice": voice, "p": p, "gens": gens, "parent": [], "new": []}
            for k in range(args.rounds):
                for which in (("parent", "new") if k % 2 == 0 else ("new", "parent")):  # neither library always runs second
                    if which == "parent":
                        r["parent"].append(timed(voice, p, gens, args.parent_lib, old=True)["us_per_generation"])
                    else:
                        r["new"].append(timed(voice, p, gens)["us_per_generation"])
            r["new_median"], r["parent_median"] = statistics.median(r["new"]), statistics.median(r["parent"])
            r["parent_spread"] = round(max(r["parent"]) - min(r["parent"]), 3)
            r["accepted"] = bool(r["new_median"] <= r["parent_median"] + r["parent_spread"])
            result["b_fixed_against_parent"].append(r)
            print(json.dumps(r), flush=True)
    else:
        result["b_fixed_against_parent"] = "not yet taken (no --parent-lib)"
    for voice in QUALITY:
        q = child(["--leg", "quality", "--voice", voice, "--gens", "1000"])
        result["c_64_shipped_chunks"].append(q)
        print(json.dumps(q), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
