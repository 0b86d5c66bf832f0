"""What rendering a whole match costs (sots_render_overlap_add), against the synthesis of the same rows.

4096 chunks of the shipped voice (3-op, N = 2048), random genes, rendered at hop N (rectangular), N/2 and N/4 (windowed):
wall time of the blocking call - genes to the device, the synthesis of every pass (rows that straddle a pass boundary
again), the gather kernel, the samples back - median of --reps repetitions after a warm-up.  Beside it the synthesis launch
of the same 4096 rows alone, on the same device in the same process: one context of P = 4096 holding the rows,
sots_stage_synthesise, as its hipEvent time (stage timing) and as wall time with the synchronise.  No time is fixed in
advance: the record states render time against that synthesis time.

    python tools/render_bench.py --out profiles/r13_render.json
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd"
PMAX = [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0]
KIND, LOG2N, DIMS = 1, 11, 6
STAGE_SYNTHESISE = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rows-per-pass", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    n, rows = 1 << LOG2N, args.chunks
    values = np.random.default_rng(13).uniform(0.05, 0.95, (rows, DIMS)).astype(np.float32)

    es = pkg.HipES(rows // 2, rows - rows // 2, synth_kind=KIND, audio_log2=LOG2N, param_max=PMAX, workgroup_size=32)
    es.write_population(values=values)
    for _ in range(3):
        es.synthesise()
    es.synchronize()
    es.timing_enable(True)
    es.timing_reset()
    wall = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        es.synthesise()
        es.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    total_ms, count = es.stage_time_ms(STAGE_SYNTHESISE)
    es.timing_enable(False)
    synth = dict(event_ms=total_ms / count, wall_ms=statistics.median(wall), launches=count)

    renders = []
    for hop, windowed in ((n, False), (n // 2, True), (n // 4, True)):
        for _ in range(2):
            out = es.render_overlap_add(values, hop, windowed=windowed, rows_per_pass=args.rows_per_pass)
        reps = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = es.render_overlap_add(values, hop, windowed=windowed, rows_per_pass=args.rows_per_pass)
            reps.append((time.perf_counter() - t0) * 1e3)
        ms = statistics.median(reps)
        renders.append(dict(hop=hop, windowed=windowed, samples=int(out.size), render_wall_ms=ms, min_ms=min(reps), max_ms=max(reps),
                            against_synthesis_event=ms / synth["event_ms"], against_synthesis_wall=ms / synth["wall_ms"],
                            seconds_of_audio=out.size / 44100.0))
    info = es.info()
    es.close()
    record = dict(tool="tools/render_bench.py", device=info.device_name.decode(), arch=info.arch.decode(), voice="3op_series", n=n,
                  chunks=rows, reps=args.reps, rows_per_pass=args.rows_per_pass, synthesis_of_the_same_rows=synth, renders=renders,
                  note="render_wall_ms is the blocking call (copies included); against_* = render_wall_ms / the synthesis time")
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
