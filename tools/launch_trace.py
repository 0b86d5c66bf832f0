"""Which kernels the library launches, with which grids, in every cell of the spectral launchers' kernel choice
(wave / wide / x-small / x / big, staged and fused, objective x weights, plain and segmented): for comparing two builds of
the library whose device code is identical but whose host launch code is not.

  SOTS_LIB_PATH=parent/libsots_hip.so timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d out/parent -- \
      python3 tools/launch_trace.py drive --label "parent commit" --cases out/parent_cases.json \
  && timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d out/tree -- \
      python3 tools/launch_trace.py drive --label "this tree" --cases out/tree_cases.json \
  && python3 tools/launch_trace.py compare out/parent out/parent_cases.json out/tree out/tree_cases.json --out profiles/r16_launch_trace.json

`drive` runs the cases one after the other on one stream; between two cases a tiny context runs sots_stage_window, which
no case does, so k_window marks the case boundaries in the trace.  `compare` cuts both traces at the marks and compares,
case by case, the ordered list of (kernel name, grid size, workgroup size, LDS bytes) of every dispatch; exit status 1
when they differ.  Shapes are the smallest that reach each cell; the rows that depend on the CU count scale with it."""
import argparse
import csv
import glob
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
MARK = "k_window"
PMAX_2OP = [3520.0, 8.0, 3520.0, 1.0]
MAX_BATCH_GENERATIONS = 3  # (the choice does not depend on the generation)


def drive(args):
    pkg = importlib.import_module("survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
    capi = pkg.capi
    from test_gpu_batch import CASES, PMAX, SEED, chunk_targets

    mark = pkg.HipES(16, 16, synth_kind=0, audio_log2=9, param_max=PMAX_2OP, seed=SEED, workgroup_size=16)
    mark.set_target_audio(chunk_targets(1, 512)[0])
    mark.init_population(0)
    mark.synthesise()
    cus = mark.info().compute_units
    names = []

    def case(name):
        mark.synchronize()
        mark.window()
        mark.synchronize()
        names.append(name)

    def context(log2n, p, objective=None, weights=False):
        es = pkg.HipES(p // 2, p // 2, synth_kind=0, audio_log2=log2n, param_max=PMAX_2OP, seed=SEED, workgroup_size=16)
        if objective == capi.OBJECTIVE_LOG_MAGNITUDE:
            es.set_objective(objective, 1e-3)
        if weights:
            es.set_objective_weights(np.linspace(0.5, 1.5, (1 << log2n) // 2, dtype=np.float32))
        es.set_target_audio(chunk_targets(1, 1 << log2n)[0])
        es.init_population(0)
        es.synchronize()
        return es

    def fused(es, generations):
        es.execute_generations(generations)
        es.synchronize()

    def staged(es):
        es.synthesise()
        es.fft()
        es.fitness()
        es.synchronize()

    # (log2 N, P, cell, generations): P = 16 x CUs is a row per resident wavefront of the wide kernel and more, and as
    # many 16-row workgroups as CUs; with the default selection plan the wide cell's second generation buckets its keys
    big_p = 16 * cus
    cells = [(9, 64, "wave", 1), (10, 64, "wave", 1), (10, big_p, "wide", 2), (8, 64, "x-small", 1), (11, 32, "x-small", 1),
             (12, big_p, "x", 1), (13, big_p, "x", 1), (14, 32, "big", 1)]
    for log2n, p, cell, generations in cells:
        es = context(log2n, p)
        case(f"context fused N=2^{log2n} P={p} ({cell})")
        fused(es, generations)
        es.close()
    for log2n, p, cell, _ in cells:
        es = context(log2n, p)
        case(f"context staged N=2^{log2n} P={p} ({cell})")
        staged(es)
        es.close()
    for log2n, p in ((10, 64), (11, 32), (14, 32)):
        for objective in (capi.OBJECTIVE_MAGNITUDE, capi.OBJECTIVE_LOG_MAGNITUDE):
            for weights in (False, True):
                es = context(log2n, p, objective, weights)
                case(f"objective {objective} weights {int(weights)} N=2^{log2n} P={p}")
                fused(es, 1)
                staged(es)
                es.close()

    def batch(name, kind, log2n, parents, offspring, chunks, generations, first, objective=None, weights=False):
        b = pkg.HipBatch(chunks, parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=16)
        if objective is not None:
            b.set_objective(objective, 1e-3)
        if weights:
            b.set_objective_weights(np.linspace(0.5, 1.5, (1 << log2n) // 2, dtype=np.float32))
        b.set_target_audio(chunk_targets(chunks, 1 << log2n))
        b.init_population(first)
        b.synchronize()
        case(name)
        b.execute_generations(min(generations, MAX_BATCH_GENERATIONS))
        b.synchronize()
        b.close()

    for kind, log2n, parents, offspring, chunks, generations, first in CASES:
        batch(f"batch voice {kind} N=2^{log2n} P={parents + offspring} chunks={chunks}", kind, log2n, parents, offspring, chunks, generations, first)
    batch("batch voice 1 N=2^11 P=32 chunks=5 log objective, weights", 1, 11, 16, 16, 5, 3, 0, capi.OBJECTIVE_LOG_MAGNITUDE, True)
    case("end")
    mark.close()
    with open(args.cases, "w") as f:
        json.dump({"library": args.label, "compute_units": cus, "cases": names[:-1]}, f, indent=1)
    print(f"{len(names) - 1} cases on {cus} CUs")


def dispatches(trace_dir):
    """[(kernel name, grid, workgroup, LDS bytes)] of a rocprofv3 --kernel-trace CSV, in dispatch order"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"{trace_dir}: expected one *kernel_trace.csv, found {files}")
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))

    def field(row, *keys):
        for k in keys:
            if k in row:
                return int(row[k])
        raise SystemExit(f"{files[0]}: none of the columns {keys}")

    def size(row, stem):
        if stem in row:
            return (int(row[stem]),)
        return tuple(int(row[f"{stem}_{axis}"]) for axis in "XYZ")

    rows.sort(key=lambda r: field(r, "Dispatch_Id", "Start_Timestamp"))
    return [(r["Kernel_Name"], size(r, "Grid_Size"), size(r, "Workgroup_Size"), field(r, "LDS_Block_Size", "Group_Segment_Size"))
            for r in rows]


def by_case(trace_dir, cases_file):
    with open(cases_file) as f:
        meta = json.load(f)
    runs, current = [], None
    for d in dispatches(trace_dir):
        if MARK in d[0]:
            current = []
            runs.append(current)
        elif current is not None:
            current.append(d)
    runs = runs[:-1]  # (what follows the mark behind the last case)
    if len(runs) != len(meta["cases"]):
        raise SystemExit(f"{trace_dir}: {len(runs)} marked runs for {len(meta['cases'])} cases")
    return meta, runs


def compare(args):
    meta_a, runs_a = by_case(args.trace_a, args.cases_a)
    meta_b, runs_b = by_case(args.trace_b, args.cases_b)
    if meta_a["cases"] != meta_b["cases"] or meta_a["compute_units"] != meta_b["compute_units"]:
        raise SystemExit("the two runs did not drive the same cases on the same device")
    cases, equal = [], True
    for name, a, b in zip(meta_a["cases"], runs_a, runs_b):
        same = a == b
        equal = equal and same
        entry = {"case": name, "equal": same,
                 "dispatches": [{"kernel": k, "grid": list(g), "workgroup": list(w), "lds": lds} for k, g, w, lds in a]}
        if not same:
            entry["dispatches_b"] = [{"kernel": k, "grid": list(g), "workgroup": list(w), "lds": lds} for k, g, w, lds in b]
        cases.append(entry)
        print(f"{'same     ' if same else 'DIFFERENT'} {len(a):4d} dispatches  {name}")
    result = {"what": "ordered (kernel, grid, workgroup, LDS bytes) of every dispatch per case, rocprofv3 --kernel-trace, library a against library b",
              "library_a": meta_a["library"], "library_b": meta_b["library"], "compute_units": meta_a["compute_units"],
              "equal": equal, "cases": cases}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print("all cases equal" if equal else "the launches differ")
    return 0 if equal else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="mode", required=True)
    d = sub.add_parser("drive")
    d.add_argument("--cases", required=True, help="JSON written: the names of the cases in the order they ran")
    d.add_argument("--label", default=os.path.basename(os.environ.get("SOTS_LIB_PATH", "libsots_hip.so")), help="what to call this library in the result")
    c = sub.add_parser("compare")
    c.add_argument("trace_a"), c.add_argument("cases_a"), c.add_argument("trace_b"), c.add_argument("cases_b")
    c.add_argument("--out")
    args = ap.parse_args()
    sys.exit(drive(args) if args.mode == "drive" else compare(args))


if __name__ == "__main__":
    main()
