"""What the chunk queue (sots_batch_queue_run) buys over today's batch-by-batch schedule, and what its slot table and
turnover cost per generation.  bench.py is left alone; this tool times whole matching runs of M chunks through S slots.

Schedules:
  a : today's, through the unchanged API - batches of S chunks; per batch, blocks of check_interval generations
      (sots_batch_execute_until) until every chunk's rule has held once, each chunk's result taken at the first boundary at
      which ITS rule holds (what Evolutionary_Strategy_HIP::matchChunksInFlight does)
  b : one sots_batch_queue_run
Workloads:
  shipped : 3-op, N = 2048, P = 16 + 16, M = 1024 noisy chunks (tools/track_overhead.py's targets), S = 64 and S = 256
  params  : parameters.json's shape, 2-op, N = 1024, P = 512 + 512, M = 256, S = 16
Rules: stall 50 / 100 / 200 looked at every 25 generations, at most 1000; and one fitness target, the median best-ever
fitness of the fixed-1000 run of the same job.

Every timed leg is a child process; the clocks settle under the workload first; a and b alternate for --rounds rounds.
Per leg: chunks/s, global generations, us per global generation, occupancy = chunk generations / (S x global generations),
and a digest of the per-chunk results, which must be the same for both schedules.  With rule = NULL the queue's us per global
generation stands against sots_batch_execute_generations on the same handle (the cost of the slot table and the turnover),
and with --parent-lib the plain batch loop and BASELINE configs[2] are timed on the parent commit's library and on this
one through tools/track_overhead.py's legs (code outside the queue did not move: the new median inside the parent's spread).

    python tools/queue_bench.py --parent-lib /path/to/parent/libsots_hip.so --out profiles/r09_queue_bench.json
    python tools/queue_bench.py --leg b --workload shipped --slots 64 --stall 50      # one leg (for a profiler run)
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from track_overhead import PMAX, targets  # noqa: E402

PKG = "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd"
WORKLOADS = {
    "shipped": dict(kind=1, log2n=11, parents=16, offspring=16, chunks=1024, slots=(64, 256), block=32),
    "params": dict(kind=0, log2n=10, parents=512, offspring=512, chunks=256, slots=(16,), block=32),
}
INTERVAL, MAX_G = 25, 1000


def make(pkg, w, slots):
    b = pkg.HipBatch(slots, w["parents"], w["offspring"], synth_kind=w["kind"], audio_log2=w["log2n"], param_max=PMAX[w["kind"]],
                     workgroup_size=w["block"])
    b.track()
    return b


def settle(b, tg, slots, seconds):
    b.set_target_audio(tg[:slots])
    b.init_population(0)
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end:
        b.execute_generations(200)
        b.synchronize()


def schedule_a(pkg, b, tg, slots, rule_kw):
    """batches of `slots` chunks through the unchanged API; returns (results, global generations)"""
    capi = pkg.capi
    rule = capi.make_stop_rule(**rule_kw)
    out = np.zeros(len(tg), capi.CHUNK_RESULT_DTYPE)
    d, global_generations = b.D, 0
    for first in range(0, len(tg), slots):
        n = min(slots, len(tg) - first)
        b.set_target_audio(tg[first:first + n])
        b.init_population(first)
        done, stopped = 0, np.zeros(n, bool)
        while done < MAX_G and not stopped.all():
            done += b.execute_until(min(INTERVAL, MAX_G - done), **rule_kw)
            v, s, f, g = b.best_ever()
            new = [c for c in range(n) if not stopped[c] and
                   (done >= MAX_G or b.L.sots_stop_rule_holds(C.byref(rule), float(f[c]), int(g[c]), done) == 1)]
            if new:
                lv, lf = b.read_best()
                for c in new:
                    r = out[first + c]
                    r["generations_run"], r["best_ever_generation"], r["best_ever_fitness"], r["last_fitness"] = done, g[c], f[c], lf[c]
                    r["best_ever_values"][:d], r["best_ever_steps"][:d], r["last_values"][:d] = v[c], s[c], lv[c]
                    stopped[c] = True
        global_generations += done
    return out, global_generations


def leg(args):
    """one process, one schedule, one rule: the whole matching run, timed once after the clocks have settled"""
    pkg = importlib.import_module(PKG)
    w = WORKLOADS[args.workload]
    chunks = args.chunks or w["chunks"]
    tg = targets(chunks, 1 << w["log2n"])
    b = make(pkg, w, args.slots)
    settle(b, tg, min(args.slots, chunks), args.settle)
    rule_kw = dict(target=args.target if args.target >= 0 else None, stall=args.stall, check_every=INTERVAL)
    if args.leg == "b":
        b.queue_targets_audio(tg)  # the targets' host transform is outside both timings (a: inside set_target_audio, see below)
    t0 = time.perf_counter()
    if args.leg == "a":
        results, global_generations = schedule_a(pkg, b, tg, args.slots, rule_kw)
    else:
        results, stats = b.queue_run(0, MAX_G, **rule_kw)
        global_generations = stats["global_generations"]
    dt = time.perf_counter() - t0
    host_transform = 0.0
    if args.leg == "a":  # the same transform, timed on its own so that it can be taken out of a's seconds
        t1 = time.perf_counter()
        b.queue_targets_audio(tg)
        host_transform = time.perf_counter() - t1
    b.close()
    chunk_generations = int(results["generations_run"].astype(np.uint64).sum())
    print(json.dumps({
        "leg": args.leg, "workload": args.workload, "slots": args.slots, "chunks": chunks, "stall": args.stall, "target": args.target,
        "seconds": round(dt, 4), "seconds_of_target_transform": round(host_transform, 4),
        "chunks_per_s": round(chunks / max(dt - host_transform, 1e-9), 1), "global_generations": int(global_generations),
        "us_per_global_generation": round((dt - host_transform) / max(1, global_generations) * 1e6, 3),
        "chunk_generations": chunk_generations,
        "occupancy": round(chunk_generations / (min(args.slots, chunks) * max(1, global_generations)), 4),
        "median_best_ever_fitness": float(np.median(results["best_ever_fitness"].astype(np.float64))),
        "results_sha256": hashlib.sha256(results.tobytes()).hexdigest()}))


def overhead_leg(args):
    """rule = NULL: the queue's us per global generation against sots_batch_execute_generations on the same handle"""
    pkg = importlib.import_module(PKG)
    w = WORKLOADS[args.workload]
    tg = targets(args.slots, 1 << w["log2n"])
    b = make(pkg, w, args.slots)
    settle(b, tg, args.slots, args.settle)
    plain, queue = [], []
    for _ in range(args.reps):
        b.set_target_audio(tg)
        b.init_population(0)
        b.synchronize()
        t0 = time.perf_counter()
        b.execute_generations(MAX_G)
        b.synchronize()
        plain.append((time.perf_counter() - t0) / MAX_G * 1e6)
        b.queue_targets_audio(tg)
        t0 = time.perf_counter()
        _, stats = b.queue_run(0, MAX_G)
        queue.append((time.perf_counter() - t0) / stats["global_generations"] * 1e6)
    b.close()
    print(json.dumps({"workload": args.workload, "slots": args.slots, "generations": MAX_G,
                      "plain_us_per_generation": round(statistics.median(plain), 3), "plain_reps": [round(x, 3) for x in plain],
                      "queue_us_per_global_generation": round(statistics.median(queue), 3), "queue_reps": [round(x, 3) for x in queue],
                      "cost_us_per_generation": round(statistics.median(queue) - statistics.median(plain), 3)}))


def child(script, extra, lib=None, timeout=900):
    env = dict(os.environ)
    if lib:
        env["SOTS_LIB_PATH"] = lib
    else:
        env.pop("SOTS_LIB_PATH", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", script)] + extra, env=env, capture_output=True, text=True, timeout=timeout)
    if out.returncode != 0:
        raise SystemExit(f"leg {extra} failed:\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def compare(name, workload, slots, rule_args, rounds, chunks):
    """a and b alternating; b must beat a by more than the spread of a's rounds"""
    legs = {"a": [], "b": []}
    base = ["--workload", workload, "--slots", str(slots)] + rule_args + (["--chunks", str(chunks)] if chunks else [])
    for k in range(rounds):
        for which in (("a", "b") if k % 2 == 0 else ("b", "a")):  # neither schedule always runs second
            legs[which].append(child("queue_bench.py", ["--leg", which] + base))
    a, b = [r["chunks_per_s"] for r in legs["a"]], [r["chunks_per_s"] for r in legs["b"]]
    digests = {r["results_sha256"] for r in legs["a"] + legs["b"]}
    out = {"rule": name, "workload": workload, "slots": slots, "a": legs["a"], "b": legs["b"],
           "a_chunks_per_s": a, "b_chunks_per_s": b, "a_spread": round(max(a) - min(a), 1),
           "b_median_over_a_median": round(statistics.median(b) / statistics.median(a), 3),
           "b_exceeds_a_by_more_than_a_spread": bool(min(b) - max(a) > max(a) - min(a)),
           "identical_results": len(digests) == 1}
    assert out["identical_results"], f"{name} {workload} S={slots}: the two schedules returned different per-chunk results"
    print(json.dumps({k: v for k, v in out.items() if k not in ("a", "b")}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["a", "b", "overhead"])
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="shipped")
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--chunks", type=int, default=0, help="fewer chunks than the workload's (a shorter job)")
    ap.add_argument("--stall", type=int, default=0)
    ap.add_argument("--target", type=float, default=-1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--settle", type=float, default=0.7, help="seconds of the workload before the timed run")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", help="libsots_hip.so built from the parent commit")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.leg == "overhead":
        return overhead_leg(args)
    if args.leg:
        return leg(args)

    result = {"what": "same device, one job; schedule a = batches of S through the unchanged API, each until every chunk's rule has held "
                      "once; b = one sots_batch_queue_run; a and b alternate, one process per leg, clocks settled under the workload; "
                      f"rules looked at every {INTERVAL} generations, at most {MAX_G}; the targets' host transform is outside both timings",
              "comparisons": [], "overhead": [], "outside_the_queue": {}}
    for workload, w in WORKLOADS.items():
        for slots in w["slots"]:
            fixed = child("queue_bench.py", ["--leg", "b", "--workload", workload, "--slots", str(slots)] +
                          (["--chunks", str(args.chunks)] if args.chunks else []))
            target = fixed["median_best_ever_fitness"]  # the fixed-1000 run of this job sets the fitness target
            result["comparisons"].append({"rule": "fixed_1000", "workload": workload, "slots": slots, "b": [fixed]})
            for name, rule_args in (("stall_50", ["--stall", "50"]), ("stall_100", ["--stall", "100"]), ("stall_200", ["--stall", "200"]),
                                    ("target_median", ["--target", repr(target)])):
                result["comparisons"].append(compare(name, workload, slots, rule_args, args.rounds, args.chunks))
            result["overhead"].append(child("queue_bench.py", ["--leg", "overhead", "--workload", workload, "--slots", str(slots)]))
            print(json.dumps(result["overhead"][-1]), flush=True)
    if args.parent_lib:
        for name in ("shipped", "c2"):  # tools/track_overhead.py's workloads: the plain batch loop (64 chunks in flight), configs[2]
            r = {"parent": [], "new": []}
            for k in range(args.rounds):
                for which in (("parent", "new") if k % 2 == 0 else ("new", "parent")):
                    extra = ["--leg", "off", "--workload", name] + (["--old-abi"] if which == "parent" else [])
                    r[which].append(child("track_overhead.py", extra, args.parent_lib if which == "parent" else None)["us_per_generation"])
            lo, hi = min(r["parent"]), max(r["parent"])
            r.update(parent_spread=[lo, hi], new_median=statistics.median(r["new"]),
                     new_inside_parent_spread=bool(lo <= statistics.median(r["new"]) <= hi),
                     new_not_above_parent_spread=bool(statistics.median(r["new"]) <= hi))
            result["outside_the_queue"][name] = r
            print(name, json.dumps(r), flush=True)
    stall = [c for c in result["comparisons"] if c["rule"].startswith("stall")]
    result["every_stall_leg_faster_by_more_than_a_spread"] = all(c["b_exceeds_a_by_more_than_a_spread"] for c in stall)
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
