"""What the phase-continuous rendering costs (sots_render_continuous) against the overlap-add rendering
(sots_render_overlap_add, 4.8) of the same track, on the same context and device.

4096 chunks of the shipped voice (3-op, N = 2048), random genes, at hop N, N/2 and N/4: wall time of the blocking calls -
genes to the device, every launch, the samples back - after untimed warm-up calls, median of --reps repetitions, the three
renderers taken in turn within each repetition.  No time is fixed in advance.  Beside the times: the bytes the continuous
renderer moves on the device per output sample as it is built (4 B of output; a stored phase word is written once and read by
the reduce and by the apply of the next stage, 12 B) against the algorithmic figure (4 B out + 8 B per stored phase word).

    python tools/render_continuous_bench.py --out profiles/r15_render_continuous.json
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
KIND, LOG2N, DIMS, OPS = 1, 11, 6, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    n, rows = 1 << LOG2N, args.chunks
    values = np.random.default_rng(15).uniform(0.05, 0.95, (rows, DIMS)).astype(np.float32)
    es = pkg.HipES(32, 32, synth_kind=KIND, audio_log2=LOG2N, param_max=PMAX, workgroup_size=32)

    algorithmic = 4 + 8 * (OPS - 1)
    as_built = 4 + 12 * (OPS - 1)
    renders = []
    for hop in (n, n // 2, n // 4):
        calls = {"overlap_add": lambda: es.render_overlap_add(values, hop, windowed=hop < n),
                 "continuous_hold": lambda: es.render_continuous(values, hop),
                 "continuous_glide": lambda: es.render_continuous(values, hop, glide=True)}
        for _ in range(args.warmup):
            for call in calls.values():
                out = call()
        times = {name: [] for name in calls}
        for _ in range(args.reps):
            for name, call in calls.items():
                t0 = time.perf_counter()
                out = call()
                times[name].append((time.perf_counter() - t0) * 1e3)
        ms = {name: statistics.median(t) for name, t in times.items()}
        samples = int(out.size)
        renders.append(dict(hop=hop, samples=samples, seconds_of_audio=samples / 44100.0, synthesised_by_overlap_add=rows * n,
                            overlap_add_ms=ms["overlap_add"], continuous_hold_ms=ms["continuous_hold"], continuous_glide_ms=ms["continuous_glide"],
                            min_ms={name: min(t) for name, t in times.items()}, max_ms={name: max(t) for name, t in times.items()},
                            hold_against_overlap_add=ms["continuous_hold"] / ms["overlap_add"],
                            glide_against_overlap_add=ms["continuous_glide"] / ms["overlap_add"],
                            hold_as_built_gb_per_s_over_call_wall=as_built * samples / ms["continuous_hold"] / 1e6))
    info = es.info()
    es.close()
    record = dict(tool="tools/render_continuous_bench.py", device=info.device_name.decode(), arch=info.arch.decode(), voice="3op_series", n=n,
                  chunks=rows, reps=args.reps, warmup=args.warmup, bytes_per_output_sample=dict(algorithmic=algorithmic, as_built=as_built),
                  renders=renders,
                  note="times are the blocking calls (copies of genes and samples included), median of reps; *_against_overlap_add = "
                       "continuous / overlap-add on the same track; as_built counts a stored phase word written once and read twice; "
                       "*_gb_per_s_over_call_wall divides by the whole call (copies and launches included): an end-to-end figure, not a kernel rate")
    text = json.dumps(record, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
