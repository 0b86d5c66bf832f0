"""What the per-bin weights of the objective (sots_set_objective_weights) cost when none are set, and what they cost set.

(a) No weights, against the parent commit.  The parent commit's libsots_hip.so (--parent-lib) and this tree's library
    alternate, --rounds rounds each in one job on one device, on tools/track_overhead.py's two workloads (c2: BASELINE
    configs[2], one context, P = 16384 + 49152, 2-op, N = 1024; shipped: 64 chunks in flight, P = 16 + 16, 3-op, N = 2048),
    --gens generations a repetition.  Accepted when the new library's median over the rounds is no higher than the
    parent's median plus the parent's own round-to-round spread (max - min): the rule of tools/survivors_bench.py and
    tools/objective_bench.py.
(b) Weighted beside unweighted, this tree's library, under MAGNITUDE and under LOG_MAGNITUDE (floor --floor): us per
    generation on c2, on the configs[3] shard (c3: one context, P = 8192 + 24576, 4-op, N = 4096) and on the shipped 64
    chunks; for the contexts also the spectral kernel's own time (hipEvent stage timing of "fused:FFT+fitness", mean per
    launch, from a second, instrumented run - the batch has no stage timers).  The weights are a band, 80 .. 6000 Hz at
    44100 Hz: what a kernel does with a weight does not depend on its value.  Report only.

us per generation = wall time of execute_generations(G) + synchronise, / G, median of --reps repetitions after --settle
seconds of the workload.  Timed by THIS tool's loop (the generation loop alone, noisy targets): not bench.py's ms_per_step.
Every leg is a child process (one process loads one library).

    python tools/objective_weights_bench.py --parent-lib /path/to/parent/libsots_hip.so --out profiles/r12_objective_weights.json
    python tools/objective_weights_bench.py --leg time --workload c3 --weights band --gens 200      # one leg (for a profiler run)
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
import track_overhead  # noqa: E402
from track_overhead import WORKLOADS, load_pkg, make  # noqa: E402

track_overhead.PMAX[3] = [3520.0, 8.0] * 4
WORKLOADS = dict(WORKLOADS, c3=dict(kind=3, log2n=12, parents=8192, offspring=24576, chunks=1, gens=200, block=32))
track_overhead.WORKLOADS = WORKLOADS


def band_weights(n, lo=80.0, hi=6000.0, rate=44100.0):
    f = np.arange(n // 2) * rate / n
    return ((f >= lo) & (f <= hi)).astype(np.float32)


def time_leg(args):
    """one process, one library, one setting: us per generation, and (contexts) the spectral kernel's time per launch"""
    pkg = load_pkg(args.old_abi)
    w = WORKLOADS[args.workload]
    gens = args.gens or w["gens"]
    es = make(pkg, w)
    if args.objective == "log":
        es.set_objective(pkg.capi.OBJECTIVE_LOG_MAGNITUDE, args.floor)
    if args.weights == "band":
        es.set_objective_weights(band_weights(1 << w["log2n"]))
    es.init_population(0)
    t_end = time.perf_counter() + args.settle  # clocks settle under the workload itself
    while time.perf_counter() < t_end:
        es.execute_generations(100)
        es.synchronize()
    reps = []
    for _ in range(args.reps):
        es.init_population(0)
        es.synchronize()
        t0 = time.perf_counter()
        es.execute_generations(gens)
        es.synchronize()
        reps.append((time.perf_counter() - t0) / gens * 1e6)
    out = {"workload": args.workload, "objective": args.objective, "weights": args.weights, "gens": gens,
           "us_per_generation": round(statistics.median(reps), 3), "reps": [round(r, 3) for r in reps], "spectral_kernel_us": None}
    if w["chunks"] == 1 and not args.old_abi:  # the instrumented run: events around every stage, so not the figure above
        es.timing_enable(True)
        es.init_population(0)
        es.timing_reset()
        es.execute_generations(gens)
        es.synchronize()
        total_ms, count = es.stage_time_ms(pkg.capi.STAGE_FUSED_SPECTRAL)
        out["spectral_kernel_us"] = round(total_ms / max(count, 1) * 1e3, 3)
        out["spectral_launches"] = count
    es.close()
    print(json.dumps(out))


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
    ap.add_argument("--leg", choices=["time"])
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="c2")
    ap.add_argument("--objective", choices=["magnitude", "log"], default="magnitude")
    ap.add_argument("--weights", choices=["none", "band"], default="none")
    ap.add_argument("--floor", type=float, default=1e-3)
    ap.add_argument("--old-abi", action="store_true")
    ap.add_argument("--gens", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of the workload before the timed repetitions")
    ap.add_argument("--parent-lib", help="libsots_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.leg == "time":
        return time_leg(args)

    common = ["--leg", "time", "--reps", str(args.reps), "--settle", str(args.settle), "--gens", str(args.gens), "--floor", str(args.floor)]
    result = {"what": "one job, one device.  (a) parent library and this tree's library alternating, no weights set, objective "
                      f"MAGNITUDE; us per generation = wall time of execute_generations({args.gens}) + synchronise, / {args.gens}, "
                      f"median of {args.reps} repetitions after {args.settle} s of the workload.  (b) this tree's library, without and "
                      f"with weights (band 80 .. 6000 Hz) under MAGNITUDE and LOG_MAGNITUDE (floor {args.floor}), timed the same way; "
                      "spectral_kernel_us = mean hipEvent time of a fused:FFT+fitness launch in a second, instrumented run (contexts "
                      "only).  Timed by this tool's own loop (the generation loop alone, noisy targets): not bench.py's ms_per_step, "
                      "not chunk_bench's us_per_generation",
              "a_unweighted_against_parent": {}, "b_weighted": {}}

    def write():
        if args.out:  # (after every step: a job that is cut short leaves what it has measured)
            with open(args.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")

    for name in ("c2", "shipped"):
        r = {"G": args.gens, "parent": [], "new": []}
        for k in range(args.rounds):
            order = ("parent", "new") if k % 2 == 0 else ("new", "parent")  # neither library always runs second
            for which in order:
                if which == "parent" and args.parent_lib:
                    r["parent"].append(child(common + ["--workload", name, "--old-abi"], args.parent_lib)["us_per_generation"])
                elif which == "new":
                    r["new"].append(child(common + ["--workload", name])["us_per_generation"])
        r["new_median"] = statistics.median(r["new"])
        if r["parent"]:
            r["parent_median"] = statistics.median(r["parent"])
            r["parent_spread"] = round(max(r["parent"]) - min(r["parent"]), 3)
            r["bound"] = round(r["parent_median"] + r["parent_spread"], 3)
            r["accepted"] = bool(r["new_median"] <= r["bound"])
        result["a_unweighted_against_parent"][name] = r
        print(name, json.dumps(r), flush=True)
        write()
    for name in ("c2", "c3", "shipped"):
        r = {}
        for objective in ("magnitude", "log"):
            for weights in ("none", "band"):
                q = child(common + ["--workload", name, "--objective", objective, "--weights", weights])
                r[f"{objective}/{weights}"] = {k: q[k] for k in ("us_per_generation", "reps", "spectral_kernel_us")}
        result["b_weighted"][name] = r
        print(name, json.dumps(r), flush=True)
        write()
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
