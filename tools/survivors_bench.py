"""What elitist survival (sots_set_survivors) costs when it is off, and what it buys when it is on.

(a) K = 0 against the parent commit.  The parent commit's libsots_hip.so (--parent-lib) and this tree's library alternate,
    --rounds rounds each in one job on one device, on tools/track_overhead.py's two workloads:
      c2      : BASELINE configs[2], bench.py's default call - one context, P = 16384 + 49152, 2-op voice, N = 1024
      shipped : the reference's shipped sizes with 64 chunks in flight - HipBatch, P = 16 + 16, 3-op voice, N = 2048
    us per generation = wall time of execute_generations(G) + synchronise, / G, median of --reps repetitions after
    --settle seconds of the workload.  Accepted when the new library's median over the rounds is no higher than the
    parent's median plus the parent's own round-to-round spread (max - min).
(b) The shipped 64 chunks x 1000 generations at K = 0, 1, 4, 16, tracked (best-ever only): us per generation (the same
    settle-repetitions-median scheme), mean and median of the final row 0 and of the best-ever fitness over the chunks.
    Report only.

The two workloads have the shapes of bench.py's default call and of tools/chunk_bench.py's 64 chunks in flight, but they
are timed by THIS tool's loop (the generation loop alone: no target set-up, no read-back, noisy targets), because a leg
must load the parent commit's library through the same Python path.  Its figures compare the two libraries with each
other; they are not bench.py's ms_per_step nor chunk_bench's us_per_generation.

Every leg is a child process (one process loads one library).

    python tools/survivors_bench.py --parent-lib /path/to/parent/libsots_hip.so --out profiles/r10_survivors.json
    python tools/survivors_bench.py --leg time --workload c2 --survivors 0 --gens 200     # one leg (for a profiler run)
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
from track_overhead import WORKLOADS, load_pkg, make  # noqa: E402

SURVIVORS = (0, 1, 4, 16)


def time_leg(args):
    """one process, one library, one K: us per generation, median and every repetition"""
    pkg = load_pkg(args.old_abi)
    w = WORKLOADS[args.workload]
    gens = args.gens or w["gens"]
    es = make(pkg, w)
    if args.survivors:
        es.set_survivors(args.survivors)
    es.init_population(0)
    t_end = time.perf_counter() + args.settle  # clocks settle under the workload itself
    while time.perf_counter() < t_end:
        es.execute_generations(200)
        es.synchronize()
    reps = []
    for _ in range(args.reps):
        es.init_population(0)
        es.synchronize()
        t0 = time.perf_counter()
        es.execute_generations(gens)
        es.synchronize()
        reps.append((time.perf_counter() - t0) / gens * 1e6)
    es.close()
    print(json.dumps({"workload": args.workload, "survivors": args.survivors, "gens": gens,
                      "us_per_generation": round(statistics.median(reps), 3), "reps": [round(r, 3) for r in reps]}))


def quality_leg(args):
    """the shipped workload, 64 chunks in flight, tracked: what the run reports after G generations with K survivors"""
    pkg = load_pkg(False)
    w = WORKLOADS["shipped"]
    gens = args.gens or w["gens"]
    b = make(pkg, w)
    b.track()
    if args.survivors:
        b.set_survivors(args.survivors)
    b.init_population(0)
    t_end = time.perf_counter() + args.settle
    while time.perf_counter() < t_end:
        b.execute_generations(200)
        b.synchronize()
    reps = []
    for _ in range(args.reps):  # every repetition is the same run: the last one's population is reported
        b.init_population(0)
        b.synchronize()
        t0 = time.perf_counter()
        b.execute_generations(gens)
        b.synchronize()
        reps.append((time.perf_counter() - t0) / gens * 1e6)
    last = b.read_best()[1].astype(np.float64)
    ever = b.best_ever()[2].astype(np.float64)
    b.close()
    print(json.dumps({"survivors": args.survivors, "chunks": w["chunks"], "gens": gens, "us_per_generation": round(statistics.median(reps), 3),
                      "reps": [round(r, 3) for r in reps],
                      "final_row0_mean": float(last.mean()), "final_row0_median": float(np.median(last)),
                      "best_ever_mean": float(ever.mean()), "best_ever_median": float(np.median(ever)),
                      "chunks_where_final_row0_is_worse_than_best_ever": int(np.sum(last > ever))}))


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
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="c2")
    ap.add_argument("--survivors", type=int, default=0)
    ap.add_argument("--old-abi", action="store_true")
    ap.add_argument("--gens", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of the workload before the timed repetitions")
    ap.add_argument("--parent-lib", help="libsots_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.leg == "time":
        return time_leg(args)
    if args.leg == "quality":
        return quality_leg(args)

    result = {"what": "one job, one device.  (a) parent library and this tree's library alternating with K = 0; us per generation = "
                      f"wall time of execute_generations(G) + synchronise, / G, median of {args.reps} repetitions after "
                      f"{args.settle} s of the workload.  (b) shipped workload, 64 chunks in flight, tracked, K = 0, 1, 4, 16, timed "
                      "the same way.  c2 and shipped have the shapes of bench.py's default call and of tools/chunk_bench.py's 64 chunks "
                      "in flight, timed by this tool's own loop (the generation loop alone, noisy targets): not bench.py's "
                      "ms_per_step, not chunk_bench's us_per_generation",
              "a_cost_with_no_survivors": {}, "b_shipped_64_chunks": []}
    common = ["--reps", str(args.reps), "--settle", str(args.settle)]
    for name in WORKLOADS:
        r = {"G": WORKLOADS[name]["gens"], "parent": [], "new": []}
        for k in range(args.rounds):
            order = ("parent", "new") if k % 2 == 0 else ("new", "parent")  # neither library always runs second
            for which in order:
                if which == "parent" and args.parent_lib:
                    r["parent"].append(child(["--leg", "time", "--workload", name, "--old-abi"] + common, args.parent_lib)["us_per_generation"])
                elif which == "new":
                    r["new"].append(child(["--leg", "time", "--workload", name] + common)["us_per_generation"])
        r["new_median"] = statistics.median(r["new"])
        if r["parent"]:
            r["parent_median"] = statistics.median(r["parent"])
            r["parent_spread"] = round(max(r["parent"]) - min(r["parent"]), 3)
            r["bound"] = round(r["parent_median"] + r["parent_spread"], 3)
            r["accepted"] = bool(r["new_median"] <= r["bound"])
        result["a_cost_with_no_survivors"][name] = r
        print(name, json.dumps(r), flush=True)
    for k in SURVIVORS:
        q = child(["--leg", "quality", "--survivors", str(k)] + common)
        result["b_shipped_64_chunks"].append(q)
        print(json.dumps(q), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
