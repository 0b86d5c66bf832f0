"""What the run record (sots_track: best-ever individual, history, stop rules) costs per generation, and what a stall
rule buys on the shipped workload.  bench.py is left alone; this tool times the generation loop itself.

Two workloads:
  c2       : BASELINE configs[2] - one context, P = 16384 + 49152, 2-op voice, N = 1024
  shipped  : the reference's shipped sizes with 64 chunks in flight - HipBatch, P = 16 + 16, 3-op voice, N = 2048
Modes: off | best_ever | history_1 | history_100 (a record every generation / every 100th).

Every timed leg is a child process (one process loads one library).  With --parent-lib the parent commit's
libsots_hip.so (tracking off - it has no tracking) alternates with this tree's library, mode off, for --rounds rounds
on the same device with settled clocks; the condition is that "new, off" lies inside the parent-against-parent spread.
The tracked modes follow, then the shipped workload matched with a stall rule against the fixed 1000 generations.

    python tools/track_overhead.py --parent-lib /path/to/parent/libsots_hip.so --out profiles/r07_track_overhead.json
    python tools/track_overhead.py --leg off --workload c2 --gens 200     # one leg (for a profiler run)
"""
from __future__ import annotations

import argparse
import ctypes
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
PKG = "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd"
PMAX = {0: [3520.0, 8.0, 3520.0, 1.0], 1: [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0]}
WORKLOADS = {
    "c2": dict(kind=0, log2n=10, parents=16384, offspring=49152, chunks=1, gens=2000, block=32),
    "shipped": dict(kind=1, log2n=11, parents=16, offspring=16, chunks=64, gens=1000, block=32),
}
MODES = {"off": None, "best_ever": dict(history_every=0), "history_1": dict(history_every=1, capacity=1024),
         "history_100": dict(history_every=100, capacity=1024)}


def load_pkg(old_abi):
    """old_abi: the library of a commit without the run record - its missing symbols become stubs that refuse to be
    called, so that the binding loads and the untracked loop can be timed through the same Python path"""
    if old_abi:
        class Missing:
            def __init__(self, name):
                self.name = name

            def __call__(self, *a):
                raise RuntimeError(f"{self.name} is not in this library")

        class Tolerant(ctypes.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if not name.startswith("sots_"):
                        raise
                    stub = Missing(name)
                    setattr(self, name, stub)
                    return stub

        ctypes.CDLL = Tolerant
    return importlib.import_module(PKG)


def targets(chunks, n):
    t = np.arange(n) / 44100.0
    out = np.empty((chunks, n), np.float32)
    for c in range(chunks):
        rng = np.random.default_rng(c)
        f = 110.0 * (1 + c % 13)
        out[c] = (0.6 * np.sin(2 * np.pi * f * t) + 0.3 * np.sin(2 * np.pi * 2.7 * f * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return out


def make(pkg, w):
    kw = dict(synth_kind=w["kind"], audio_log2=w["log2n"], param_max=PMAX[w["kind"]], workgroup_size=w["block"])
    tg = targets(w["chunks"], 1 << w["log2n"])
    if w["chunks"] == 1:
        es = pkg.HipES(w["parents"], w["offspring"], **kw)
        es.set_target_audio(tg[0])
    else:
        es = pkg.HipBatch(w["chunks"], w["parents"], w["offspring"], **kw)
        es.set_target_audio(tg)
    return es


def leg(args):
    """one process, one library, one mode: us per generation, median and every repetition"""
    pkg = load_pkg(args.old_abi)
    w = WORKLOADS[args.workload]
    gens = args.gens or w["gens"]
    es = make(pkg, w)
    if MODES[args.leg] is not None:
        es.track(**MODES[args.leg])
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
    print(json.dumps({"leg": args.leg, "workload": args.workload, "gens": gens, "us_per_generation": round(statistics.median(reps), 3),
                      "reps": [round(r, 3) for r in reps]}))


def stop_leg(args):
    """the shipped workload, 64 chunks in flight: the fixed 1000 generations against stall rules"""
    pkg = load_pkg(False)
    w = WORKLOADS["shipped"]
    tg = targets(w["chunks"], 1 << w["log2n"])
    b = make(pkg, w)
    b.track()
    out = {}
    for name, stall in (("fixed_1000", 0), ("stall_50", 50), ("stall_100", 100), ("stall_200", 200)):
        for timed in (False, True):  # the first pass warms up
            t0 = time.perf_counter()
            b.set_target_audio(tg)
            b.init_population(0)
            if stall:
                run = b.execute_until(w["gens"], stall=stall, check_every=25)
            else:
                b.execute_generations(w["gens"])
                run = w["gens"]
            b.synchronize()
            _, _, ever, _ = b.best_ever()
            _, last = b.read_best()
            dt = time.perf_counter() - t0
        out[name] = {"generations_run": run, "seconds": round(dt, 4), "chunks_per_s": round(w["chunks"] / dt, 1),
                     "mean_best_ever_fitness": float(np.mean(ever.astype(np.float64))),
                     "mean_last_row0_fitness": float(np.mean(last.astype(np.float64))),
                     "chunks_where_last_row0_is_worse": int(np.sum(last > ever))}
    b.close()
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
    ap.add_argument("--leg", choices=sorted(MODES) + ["stop"])
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="c2")
    ap.add_argument("--old-abi", action="store_true")
    ap.add_argument("--gens", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of the workload before the timed repetitions")
    ap.add_argument("--parent-lib", help="libsots_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.leg == "stop":
        return stop_leg(args)
    if args.leg:
        return leg(args)

    result = {"what": "same device, one job: parent library and this tree's library alternating with tracking off, then the "
                      "tracked modes; us per generation = wall time of execute_generations(G) + synchronise, / G, median of "
                      f"{args.reps} repetitions after {args.settle} s of the workload", "workloads": {}}
    for name in WORKLOADS:
        r = {"G": WORKLOADS[name]["gens"], "parent_off": [], "new_off": []}
        for k in range(args.rounds):
            order = ("parent", "new") if k % 2 == 0 else ("new", "parent")  # neither library always runs second
            for which in order:
                if which == "parent" and args.parent_lib:
                    r["parent_off"].append(child(["--leg", "off", "--workload", name, "--old-abi"], args.parent_lib)["us_per_generation"])
                elif which == "new":
                    r["new_off"].append(child(["--leg", "off", "--workload", name])["us_per_generation"])
        for mode in ("best_ever", "history_1", "history_100"):
            r[mode] = child(["--leg", mode, "--workload", name])["us_per_generation"]
        if r["parent_off"]:
            lo, hi = min(r["parent_off"]), max(r["parent_off"])
            r["parent_spread"] = [lo, hi]
            r["new_off_median"] = statistics.median(r["new_off"])
            r["new_off_inside_parent_spread"] = bool(lo <= r["new_off_median"] <= hi)
            r["new_off_not_above_parent_spread"] = bool(r["new_off_median"] <= hi)
        base = statistics.median(r["new_off"])
        r["cost_us_per_generation"] = {m: round(r[m] - base, 3) for m in ("best_ever", "history_1", "history_100")}
        result["workloads"][name] = r
        print(name, json.dumps(r), flush=True)
    result["shipped_stop_rules"] = child(["--leg", "stop"])
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
