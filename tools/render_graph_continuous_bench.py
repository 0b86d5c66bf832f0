"""What the phase-continuous rendering of the operator-graph voice costs (sots_render_graph_continuous).

4096 chunks at N = 2048, random genes, at hop N, N/2 and N/4, for the graphs 2op, triple, chain3, dense8 and additive8: wall
time of the blocking calls - genes to the device, every launch, the samples back - after untimed warm-up calls, median of
--reps repetitions, the renderers taken in turn within each repetition.  No time is fixed in advance.
  (a) the new call against sots_render_overlap_add on the same context;
  (b) for 2op and triple, the new call against sots_render_continuous of the fixed voice on the same rows: the same bits (the
      tool checks that), so the ratio is the price of generality - a phase buffer per operator and the mix launch;
  (c) one shaped setting: dense8 with one of every waveform code;
  (d) the bytes the renderer moves on the device per output sample as it is built: 4 B of output, every operator's phase word
      written once (4 B), read by the reduce and by the apply of every operator it modulates (8 B per edge of the graph) and,
      for a carrier, by the mix (4 B).

    python tools/render_graph_continuous_bench.py --out profiles/r26_render_graph_continuous.json
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
LOG2N = 11
# (operators, modulators as masks, carriers as a mask): the graphs of tests/_graph_voice_model.py
GRAPHS = {
    "2op": (2, [0, 0b1], 0b10),
    "triple": (6, [0, 0b1, 0, 0b100, 0, 0b10000], 0b101010),
    "chain3": (3, [0, 0b1, 0b10], 0b100),
    "dense8": (8, [0] + [(1 << min(j, 6)) - 1 for j in range(1, 8)], 0b11000000),
    "additive8": (8, [0] * 8, 0xFF),
}
FIXED = {"2op": 0, "triple": 2}  # the fixed voices that are these graphs
MIXED8 = [3, 1, 6, 0, 7, 4, 2, 5]
PMAX4 = [3520.0, 8.0, 3520.0, 1.0]


def ranges(graph):
    ops, _, carriers = graph
    pmax = []
    for j in range(ops):
        pmax += [3520.0, 1.0 if carriers >> j & 1 else 8.0]
    return pmax


def levels(graph):
    ops, mods, _ = graph
    lv = []
    for j in range(ops):
        lv.append(0 if mods[j] == 0 else 1 + max(lv[i] for i in range(j) if mods[j] >> i & 1))
    return max(lv) + 1


def bytes_as_built(graph):
    ops, mods, carriers = graph
    edges = sum(bin(m).count("1") for m in mods)
    return 4 + 4 * ops + 8 * edges + 4 * bin(carriers).count("1")


def timed(calls, warmup, reps):
    for _ in range(warmup):
        for call in calls.values():
            call()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: dict(median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    n, rows = 1 << LOG2N, args.chunks
    records = []
    info = None
    for name, graph in GRAPHS.items():
        ops = graph[0]
        values = np.random.default_rng(26).uniform(0.05, 0.95, (rows, 2 * ops)).astype(np.float32)
        pmax = PMAX4 * (ops // 2) if name in FIXED else ranges(graph)  # (the anchors: the ranges of genes 0..3 per pair)
        es = pkg.HipES(32, 32, synth_kind=pkg.capi.SYNTH_GRAPH, audio_log2=LOG2N, param_max=pmax, workgroup_size=32,
                       graph=pkg.capi.make_voice_graph(*graph))
        fixed = pkg.HipES(32, 32, synth_kind=FIXED[name], audio_log2=LOG2N, param_max=PMAX4, workgroup_size=32) if name in FIXED else None
        info = es.info()
        settings = [("sine", None)] + ([("mixed", MIXED8)] if name == "dense8" else [])
        for setting, waves in settings:
            es.set_voice_waveforms(waves)
            for hop in (n, n // 2, n // 4):
                calls = {"overlap_add": lambda: es.render_overlap_add(values, hop, windowed=hop < n),
                         "graph_continuous_hold": lambda: es.render_graph_continuous(values, hop),
                         "graph_continuous_glide": lambda: es.render_graph_continuous(values, hop, glide=True)}
                if fixed is not None:
                    calls["fixed_continuous_hold"] = lambda: fixed.render_continuous(values, hop)
                    same = np.array_equal(es.render_graph_continuous(values, hop).view(np.uint32), fixed.render_continuous(values, hop).view(np.uint32))
                t = timed(calls, args.warmup, args.reps)
                samples = (rows - 1) * hop + n
                rec = dict(graph=name, operators=ops, levels=levels(graph), launches_per_pass=3 * levels(graph) + 1, waveforms=setting, hop=hop,
                           samples=samples, times=t, bytes_per_output_sample_as_built=bytes_as_built(graph),
                           hold_against_overlap_add=t["graph_continuous_hold"]["median_ms"] / t["overlap_add"]["median_ms"],
                           glide_against_overlap_add=t["graph_continuous_glide"]["median_ms"] / t["overlap_add"]["median_ms"])
                if fixed is not None:
                    rec["same_bits_as_fixed_voice"] = bool(same)
                    rec["hold_against_fixed_continuous"] = t["graph_continuous_hold"]["median_ms"] / t["fixed_continuous_hold"]["median_ms"]
                records.append(rec)
                print(json.dumps(rec), flush=True)
        es.close()
        if fixed is not None:
            fixed.close()
    record = dict(tool="tools/render_graph_continuous_bench.py", device=info.device_name.decode(), arch=info.arch.decode(), n=n, chunks=rows,
                  reps=args.reps, warmup=args.warmup, renders=records,
                  note="times are the blocking calls (copies of genes and samples included), median of reps; *_against_overlap_add = the new "
                       "call / sots_render_overlap_add on the same context and track; hold_against_fixed_continuous = the new call / "
                       "sots_render_continuous of the fixed voice that the graph is (the same bits: same_bits_as_fixed_voice); "
                       "bytes_per_output_sample_as_built: 4 out + 4 per operator + 8 per edge + 4 per carrier")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(record, indent=1) + "\n")


if __name__ == "__main__":
    main()
