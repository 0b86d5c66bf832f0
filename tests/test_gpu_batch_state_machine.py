"""Random call orders on a HipBatch against one sequential context per chunk (tests/_state_machine.py, the batch part).

The batch runs a seeded list of 40 calls: target calls whose chunk counts grow and shrink, init_population, generations,
execute_until, objective, weights, survivors, tracking, host and device analysis, stored queues, carried rows, queue runs
with and without a kept chunk, every read, refused calls.  In lockstep one HipES per chunk goes through the same logical
history, as test_gpu_batch.sequential does; a queue run is checked against the sequential tracked context that the header
of sots_batch_queue_run spells out, carried rows included; under SOTS_ANALYSIS_DEVICE the contexts get
set_target_spectrum of the batch's analyse_audio_hop, as test_gpu_analysis.py has it.  A checkpoint compares every active
chunk's population, read_best, best_ever and history bit for bit.

SOTS_SM_SEED / SOTS_SM_CASES / SOTS_SM_OPS / SOTS_SM_REPLAY=<seed>:<k> / SOTS_SM_REPORT as in test_gpu_state_machine.py.
"""
import json
import os
import time

import numpy as np
import pytest

import _state_machine as SM

pytestmark = pytest.mark.gpu


def cases():
    replay = os.environ.get("SOTS_SM_REPLAY")
    n = int(os.environ.get("SOTS_SM_CASES", "8"))
    out = []
    for i, name in enumerate(SM.BATCH_SHAPES):
        if "SOTS_SM_SEED" in os.environ:
            seeds = [int(os.environ["SOTS_SM_SEED"]) + 100 * i + j for j in range(n)]
        else:
            seeds = (SM.BATCH_SEEDS[name] + [SM.BATCH_SEEDS[name][-1] + 1 + j for j in range(max(0, n - 8))])[:n]
        if replay:
            seed, k = (int(x) for x in replay.split(":"))
            out += [(name, seed, k)] if seed in seeds else []
        else:
            out += [(name, s, None) for s in seeds]
    return out


@pytest.mark.parametrize("shape,seed,k", cases())
def test_random_call_order_equals_sequential_contexts(pkg, shape, seed, k):
    sh = SM.BatchShape(shape)
    ops, _ = SM.generate_batch(shape, seed, int(os.environ.get("SOTS_SM_OPS", SM.BATCH_OPS)))
    if k is not None:
        ops = ops[:k]  # (a difference is reported by the call that finds it: a cut list needs no last checkpoint)
    t = time.time()
    batch = sh.make_batch(pkg)
    refs = [sh.make(pkg) for _ in range(sh.slots)]
    try:
        bad = SM.run_batch(batch, refs, sh, ops, lambda n: np.zeros(n, pkg.capi.CHUNK_RESULT_DTYPE))
    finally:
        batch.close()
        for r in refs:
            r.close()
    if "SOTS_SM_REPORT" in os.environ:
        line = dict(shape=shape, seed=seed, seconds=round(time.time() - t, 3), ok=bad is None)
        if bad:
            line["op_index"] = bad[0]
        with open(os.environ["SOTS_SM_REPORT"], "a") as f:
            f.write(json.dumps(line) + "\n")
    assert bad is None, (f"{shape} seed {seed}: call {bad[0]}: {bad[1]}.\nReplay with SOTS_SM_REPLAY={seed}:{bad[0] + 1}.  The calls up to there:\n"
                         + "\n".join(repr(op) for op in ops[:bad[0] + 1]))
