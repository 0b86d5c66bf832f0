"""What making the queue targets costs on the host and on the device (sots_batch_set_analysis).  bench.py is
left alone.

The call timed is sots_batch_queue_targets_audio_hop, end to end as a caller sees it: under SOTS_ANALYSIS_HOST the fp64
transform chunk by chunk on one host thread, the upload of the spectra and the derived tables; under SOTS_ANALYSIS_DEVICE the
upload of the samples, k_analyse into the stored targets and the same derived tables.  The call returns after a stream
synchronise, so a host clock around it covers upload, kernels and synchronise.  Two workloads, the shipped shape (3-op voice,
N = 2048, P = 16 + 16):
  track    4096 chunks at hop 512: the gliding track of tools/queue_carry_bench.py (the recipe of tests/_carry_model.py)
  shipped  the 64 shipped chunks at hop N (tools/track_overhead.py's noisy targets)
Each leg is a child process: one warm-up call on the same input, then --reps timed calls; the median and every repetition are
reported; the device leg also reports how far its magnitudes lie from NumPy's fp64 transform of the same frames, relative to
each frame's largest bin.  The yardstick is the host leg of the same job: no figure is fixed in advance.

    python tools/analysis_bench.py --out profiles/r21_analysis.json
    python tools/analysis_bench.py --leg device --workload track       # one leg (for a profiler run)
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
from queue_carry_bench import HOP, SHIPPED, SLOTS, gliding_track  # noqa: E402
from track_overhead import PMAX, load_pkg, targets  # noqa: E402


def workload(name, chunks):
    n = 1 << SHIPPED["log2n"]
    if name == "track":
        return gliding_track(chunks, n, HOP), HOP, chunks
    return targets(SLOTS, n).reshape(-1), n, SLOTS


def leg(args):
    """one process, one mode: seconds per sots_batch_queue_targets_audio_hop on one workload"""
    pkg = load_pkg(False)
    w = SHIPPED
    b = pkg.HipBatch(SLOTS, w["parents"], w["offspring"], synth_kind=w["kind"], audio_log2=w["log2n"], param_max=PMAX[w["kind"]],
                     workgroup_size=w["block"])
    b.track()
    x, hop, chunks = workload(args.workload, args.chunks)
    b.set_analysis(pkg.capi.ANALYSIS_DEVICE if args.leg == "device" else pkg.capi.ANALYSIS_HOST)
    b.queue_targets_audio(x, hop)   # warm-up: code objects loaded, buffers allocated
    assert b.queued == chunks
    reps = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        b.queue_targets_audio(x, hop)
        reps.append(time.perf_counter() - t0)
    out = {"mode": args.leg, "workload": args.workload, "chunks": chunks, "hop": hop, "n": 1 << w["log2n"],
           "seconds": round(statistics.median(reps), 6), "reps": [round(r, 6) for r in reps],
           "us_per_chunk": round(statistics.median(reps) / chunks * 1e6, 3), "chunks_per_s": round(chunks / statistics.median(reps), 1)}
    if args.leg == "device":   # what the mode stores, against an fp64 transform of the same frames (the first 64 chunks)
        n, k = 1 << w["log2n"], min(chunks, 64)
        got = b.analyse_audio_hop(x, hop, k).astype(np.float64)
        i = np.arange(n, dtype=np.float64)
        one_over = np.float32(1.0) / np.float32(n)
        win = 1.0 - np.cos(i * np.float64(one_over - np.float32(1.0)) * 2.0 * np.pi)
        f = np.float32(0.0)
        for v in win:
            f = np.float32(np.float64(f) + v)
        scale = np.float64(one_over) * np.float64(np.float32(1.0) / np.float32(f * one_over))
        fr = np.stack([x[c * hop:c * hop + n] for c in range(k)]).astype(np.float64) * win
        want = np.abs(np.fft.rfft(fr, axis=-1))[:, :n // 2] * scale
        out["max_error_over_largest_bin"] = float((np.abs(got - want).max(axis=1) / want.max(axis=1)).max())
    b.close()
    print(json.dumps(out))


def child(extra):
    env = dict(os.environ)
    env.pop("SOTS_LIB_PATH", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + extra, env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(f"leg {extra} failed:\n{out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["host", "device"])
    ap.add_argument("--workload", choices=["track", "shipped"], default="track")
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.leg:
        return leg(args)

    result = {"what": "one job, one device: wall time of sots_batch_queue_targets_audio_hop (it ends in a stream synchronise) under "
                      "SOTS_ANALYSIS_HOST and SOTS_ANALYSIS_DEVICE, each leg a child process, one warm-up call then the median of "
                      f"{args.reps} calls; upload and synchronise are inside the device timing, the host leg's fp64 transform runs on "
                      "one thread of the job's CPU.  This tool's own timing: not bench.py's ms_per_step",
              "legs": [], "summary": {}}
    for name in ("track", "shipped"):
        medians = {"host": [], "device": []}
        for k in range(args.rounds):
            for mode in (("host", "device") if k % 2 == 0 else ("device", "host")):   # neither mode always runs second
                q = child(["--leg", mode, "--workload", name, "--chunks", str(args.chunks), "--reps", str(args.reps)])
                result["legs"].append(q)
                medians[mode].append(q["seconds"])
                print(json.dumps(q), flush=True)
        h, d = statistics.median(medians["host"]), statistics.median(medians["device"])
        result["summary"][name] = {"host_seconds": h, "device_seconds": d, "host_over_device": round(h / d, 2),
                                   "device_faster_end_to_end": bool(d < h)}
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
