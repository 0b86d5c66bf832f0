"""Chunks in flight against the chunk-by-chunk loop (the reference's parameterMatchAudio shape).

Prints ONE JSON line with two workloads:
  shipped     : the reference's shipped sizes - P = 16 + 16, 3-op voice, N = 2048, 64 chunks, G generations (1000)
  parameters  : the repository's parameters.json - P = 256 + 768, 2-op voice, N = 1024, 16 chunks, 100 generations
and for each: the sequential HipES loop (per chunk: target, init, G generations, synchronise, best row) and HipBatch
at the listed chunk counts (per batch: targets, init, G generations, ONE synchronisation, best rows) - us per
generation (wall time / (G x launches of generations)), chunks/s, M candidates/s, the speed-up in chunks/s over the
sequential loop, and whether every chunk's best row is bit-identical to the sequential loop's.

    python tools/chunk_bench.py                                  # both workloads
    python tools/chunk_bench.py --only shipped --batch-only 64   # one batched leg (for a profiler run)
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import importlib  # noqa: E402

pkg = importlib.import_module("survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")

PMAX = {0: [3520.0, 8.0, 3520.0, 1.0], 1: [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0]}
WORKLOADS = {
    "shipped": dict(kind=1, log2n=11, parents=16, offspring=16, chunks=64, gens=1000, batches=[8, 64], block=32),
    "parameters": dict(kind=0, log2n=10, parents=256, offspring=768, chunks=16, gens=100, batches=[16], block=32),
}


def targets(chunks, n):
    t = np.arange(n) / 44100.0
    out = np.empty((chunks, n), np.float32)
    for c in range(chunks):
        f = 110.0 * (1 + c % 13)
        out[c] = (0.6 * np.sin(2 * np.pi * f * t) + 0.3 * np.sin(2 * np.pi * 2.7 * f * t)).astype(np.float32)
    return out


def sequential(w, tg, gens):
    es = pkg.HipES(w["parents"], w["offspring"], synth_kind=w["kind"], audio_log2=w["log2n"], param_max=PMAX[w["kind"]],
                   workgroup_size=w["block"])
    best = []
    t0 = time.perf_counter()
    for c, a in enumerate(tg):
        es.set_target_audio(a)
        es.init_population(c)
        es.execute_generations(gens)
        es.synchronize()
        v, _, f = es.read_population()
        best.append((v[0].copy(), f[0]))
    dt = time.perf_counter() - t0
    es.close()
    return dt, best


def batched(w, tg, gens, per_batch):
    b = pkg.HipBatch(per_batch, w["parents"], w["offspring"], synth_kind=w["kind"], audio_log2=w["log2n"],
                     param_max=PMAX[w["kind"]], workgroup_size=w["block"])
    best = []
    t0 = time.perf_counter()
    for first in range(0, len(tg), per_batch):
        b.set_target_audio(tg[first:first + per_batch])
        b.init_population(first)
        b.execute_generations(gens)
        b.synchronize()
        v, f = b.read_best()
        best += [(v[i].copy(), f[i]) for i in range(len(f))]
    dt = time.perf_counter() - t0
    b.close()
    return dt, best


def leg(dt, w, gens, launches):
    chunks, p = w["chunks"], w["parents"] + w["offspring"]
    return {"seconds": round(dt, 4), "us_per_generation": round(dt / (gens * launches) * 1e6, 2),
            "chunks_per_s": round(chunks / dt, 2), "m_candidates_per_s": round(p * gens * chunks / dt / 1e6, 3)}


def same(a, b):
    return all(np.array_equal(x[0], y[0]) and np.float32(x[1]).tobytes() == np.float32(y[1]).tobytes() for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=sorted(WORKLOADS))
    ap.add_argument("--batch-only", type=int, default=0, help="run just HipBatch with this many chunks per batch")
    ap.add_argument("--gens", type=int, default=0, help="override the workloads' generation counts")
    args = ap.parse_args()
    out = {"tool": "chunk_bench", "device": None}
    for name, w in WORKLOADS.items():
        if args.only and name != args.only:
            continue
        gens = args.gens or w["gens"]
        tg = targets(w["chunks"], 1 << w["log2n"])
        batched(w, tg[:2], 2, 2)  # warm-up: code objects, occupancy queries
        r = {"P": w["parents"] + w["offspring"], "voice": w["kind"], "N": 1 << w["log2n"], "chunks": w["chunks"], "G": gens}
        if args.batch_only:
            dt, _ = batched(w, tg, gens, args.batch_only)
            r[f"batch_{args.batch_only}"] = leg(dt, w, gens, -(-w["chunks"] // args.batch_only))
        else:
            sequential(w, tg[:1], 2)
            dt_s, best_s = sequential(w, tg, gens)
            r["sequential"] = leg(dt_s, w, gens, w["chunks"])
            for c in w["batches"]:
                dt_b, best_b = batched(w, tg, gens, c)
                r[f"batch_{c}"] = leg(dt_b, w, gens, -(-w["chunks"] // c))
                r[f"batch_{c}"]["speedup_chunks_per_s"] = round(dt_s / dt_b, 2)
                r[f"batch_{c}"]["best_rows_bit_identical"] = bool(same(best_s, best_b))
        out[name] = r
    es = pkg.HipES(16, 16, param_max=PMAX[0])
    out["device"] = es.info().arch.decode()
    es.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
