"""What carried rows in the chunk queue (sots_batch_queue_set_carry) cost when they are off, and what they
buy on a long gliding track when they are on.  bench.py is left alone.

(a) Carry off against the parent commit.  The parent commit's libsots_hip.so (--parent-lib) and this tree's library
    alternate, --rounds rounds each in one job on one device, on the queue loop of the 64 shipped chunks (3-op voice,
    N = 2048, P = 16 + 16, tools/track_overhead.py's noisy targets) in 64 slots with rule = NULL: us per loop generation =
    wall time of sots_batch_queue_run(1000 generations) / the loop generations it reports, median of --reps repetitions
    after --settle seconds of the workload.  Accepted when the new library's median over the rounds is no higher than the
    parent's median plus the parent's own round-to-round spread (max - min).
(b) A long gliding track: one tone gliding an octave per 2 s from 330 Hz - the recipe of tests/_carry_model.py, restated here
    so that a tool does not import a test; beyond the 4 s at which it would leave the audible range the glide turns and comes
    down again at the same rate - with its octave and a little noise, --chunks chunks (4096) at hop 512, one survivor, a
    50-generation stall looked at every 25 generations, at most 1000, in 64 slots.  With nothing carried (R = 0) and with
    R = 1 at a few segment lengths L: chunks/s, the sum of generations_run, the mean best-ever fitness and the mean
    |difference| of the best-ever genes of neighbouring chunks (seams between segments included).  Report only.

Every leg is a child process (one process loads one library); the targets' host transform is outside every timing.

    python tools/queue_carry_bench.py --parent-lib /path/to/parent/libsots_hip.so --out profiles/r20_queue_carry.json
    python tools/queue_carry_bench.py --leg track --rows 1 --segment 64        # one leg (for a profiler run)
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from track_overhead import PMAX, load_pkg, targets  # noqa: E402

SHIPPED = dict(kind=1, log2n=11, parents=16, offspring=16, block=32)
SLOTS, MAX_G, HOP = 64, 1000, 512
STALL = dict(target=None, stall=50, check_every=25)
SEGMENTS = (16, 64, 256)
TURN_SECONDS = 4.0  # two octaves up, 330 Hz -> 1320 Hz, then down again


def gliding_track(chunks, n=2048, hop=HOP):
    total = (chunks - 1) * hop + n
    t = np.arange(total) / 44100.0
    up = np.abs((t + TURN_SECONDS) % (2.0 * TURN_SECONDS) - TURN_SECONDS)  # t up to the turn, then back down to 0, and again
    f = 330.0 * 2.0 ** (up / 2.0)
    phase = 2.0 * np.pi * np.cumsum(f) / 44100.0
    x = 0.6 * np.sin(phase) + 0.3 * np.sin(2.0 * phase) + 0.02 * np.random.default_rng(7).standard_normal(total)
    return x.astype(np.float32)


def make(pkg):
    w = SHIPPED
    b = pkg.HipBatch(SLOTS, w["parents"], w["offspring"], synth_kind=w["kind"], audio_log2=w["log2n"], param_max=PMAX[w["kind"]],
                     workgroup_size=w["block"])
    b.track()
    return b


def settle(b, seconds):
    """the clocks settle under the workload itself: the plain batch loop on 64 noisy chunks"""
    b.set_target_audio(targets(SLOTS, 1 << SHIPPED["log2n"]))
    b.init_population(0)
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end:
        b.execute_generations(200)
        b.synchronize()


def loop_leg(args):
    """one process, one library, carry off: us per loop generation of the queue loop on the 64 shipped chunks"""
    pkg = load_pkg(args.old_abi)
    b = make(pkg)
    settle(b, args.settle)
    b.queue_targets_audio(targets(SLOTS, 1 << SHIPPED["log2n"]))
    reps, digests = [], set()
    for _ in range(args.reps):
        t0 = time.perf_counter()
        results, stats = b.queue_run(0, MAX_G)
        reps.append((time.perf_counter() - t0) / stats["global_generations"] * 1e6)
        digests.add(hashlib.sha256(results.tobytes()).hexdigest())
    b.close()
    assert len(digests) == 1
    print(json.dumps({"us_per_loop_generation": round(statistics.median(reps), 3), "reps": [round(r, 3) for r in reps],
                      "loop_generations": int(stats["global_generations"]), "results_sha256": digests.pop()}))


def track_leg(args):
    """one process: the gliding track through the queue with R = args.rows carried rows in segments of args.segment"""
    pkg = load_pkg(False)
    b = make(pkg)
    settle(b, args.settle)
    b.set_survivors(1)
    b.queue_set_carry(args.rows, args.segment)
    b.queue_targets_audio(gliding_track(args.chunks), hop=HOP)
    assert b.queued == args.chunks
    t0 = time.perf_counter()
    results, stats = b.queue_run(0, MAX_G, **STALL)
    dt = time.perf_counter() - t0
    b.close()
    genes = results["best_ever_values"][:, :b.D].astype(np.float64)
    print(json.dumps({
        "carry_rows": args.rows, "segment_chunks": args.segment if args.rows else 0, "chunks": args.chunks, "slots": stats["slots"],
        "seconds": round(dt, 4), "chunks_per_s": round(args.chunks / dt, 1), "loop_generations": int(stats["global_generations"]),
        "sum_generations_run": int(stats["chunk_generations"]),
        "mean_best_ever_fitness": float(results["best_ever_fitness"].astype(np.float64).mean()),
        "mean_abs_gene_difference_between_neighbours": float(np.abs(np.diff(genes, axis=0)).mean()),
        "results_sha256": hashlib.sha256(results.tobytes()).hexdigest()}))


def child(extra, lib=None):
    env = dict(os.environ)
    if lib:
        env["SOTS_LIB_PATH"] = lib
    else:
        env.pop("SOTS_LIB_PATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(f"leg {extra} failed:\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["loop", "track"])
    ap.add_argument("--old-abi", action="store_true")
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--segment", type=int, default=0)
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--settle", type=float, default=1.0, help="seconds of the workload before the timed runs")
    ap.add_argument("--parent-lib", help="libsots_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.leg == "loop":
        return loop_leg(args)
    if args.leg == "track":
        return track_leg(args)

    result = {"what": "one job, one device.  (a) the queue loop of the 64 shipped chunks in 64 slots, rule = NULL, carry off: parent "
                      "library and this tree's library alternating; us per loop generation = wall time of sots_batch_queue_run(1000) / "
                      f"its loop generations, median of {args.reps} repetitions after {args.settle} s of the workload.  (b) the gliding "
                      f"track, {args.chunks} chunks at hop {HOP}, one survivor, stall 50 looked at every 25, at most {MAX_G} generations, "
                      "64 slots; the targets' host transform is outside every timing.  This tool's own loops: not bench.py's ms_per_step",
              "a_queue_loop_with_carry_off": {}, "b_gliding_track": []}
    common = ["--reps", str(args.reps), "--settle", str(args.settle)]
    r = {"parent": [], "new": [], "digests": set()}
    for k in range(args.rounds):
        order = ("parent", "new") if k % 2 == 0 else ("new", "parent")  # neither library always runs second
        for which in order:
            if which == "parent" and not args.parent_lib:
                continue
            leg = child(["--leg", "loop"] + (["--old-abi"] if which == "parent" else []) + common, args.parent_lib if which == "parent" else None)
            r[which].append(leg["us_per_loop_generation"])
            r["digests"].add(leg["results_sha256"])
    r["identical_results"] = len(r.pop("digests")) == 1
    r["new_median"] = statistics.median(r["new"])
    if r["parent"]:
        r["parent_median"] = statistics.median(r["parent"])
        r["parent_spread"] = round(max(r["parent"]) - min(r["parent"]), 3)
        r["bound"] = round(r["parent_median"] + r["parent_spread"], 3)
        r["accepted"] = bool(r["new_median"] <= r["bound"])
    result["a_queue_loop_with_carry_off"] = r
    print(json.dumps(r), flush=True)
    for rows, segment in [(0, 0)] + [(1, l) for l in SEGMENTS]:
        q = child(["--leg", "track", "--rows", str(rows), "--segment", str(segment), "--chunks", str(args.chunks), "--settle", str(args.settle)])
        result["b_gliding_track"].append(q)
        print(json.dumps(q), flush=True)
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
