"""Random call orders on the C-ABI context against a replay (tests/_state_machine.py has the generator, the legality
rules and the normaliser; tests/test_state_machine_cpu.py checks those without a GPU).

A, the subject, runs a seeded list of 60 calls as drawn: fused and staged generations, execute_until, sort modes, select
plans, hand-written splitter slots, bucket_fitness + select + rotate, targets, objectives, weights, survivors, arithmetic,
voice settings, init / write / inject, stage groups, every read, renderings, tracking on and off, refused calls.
B, the reference, is a fresh context that runs the same logical history by the plainest path the library has: SORT_FULL,
SELECT_TILES, one execute_generation() per generation, nothing else.  B's path is the one the parity tests tie to the
oracle, so A == B, bit for bit at every checkpoint, says that nothing the context keeps between calls leaks into results.
C, a second reference, runs B's list too, but meets every landscape on a FRESH context: at a target, objective, weights or
voice setter it reads its population out, makes a new context, applies the settings in force once, writes the population
and the generation counter back (the header's resume path; such a setter clears the run record anyway) and goes on.  A and
B run the same incremental rules of derive_target on the same history, so a rule that is wrong on both sides - a table not
rebuilt for the second target, a record not cleared - shows only against C, which has never had a first target.

A checkpoint compares read_population (all rows, or rows 0..S-1 where SORT_TOP_ONLY leaves the rest unspecified),
read_target, every getter, best_ever and history(with_taken=True), as bits (a NaN equals a NaN of the same bits), and
the generations every execute_until since the last checkpoint returned.

SOTS_SM_SEED / SOTS_SM_CASES draw other or more sequences, SOTS_SM_OPS changes their length, and
SOTS_SM_REPLAY=<seed>:<k> runs the first k calls of that seed's sequence (of the shape whose seeds contain it, or of every
shape with SOTS_SM_SEED).  SOTS_SM_REPORT=<file> appends one JSON line per case: shape, seed, seconds, outcome.
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
    n = int(os.environ.get("SOTS_SM_CASES", "12"))
    out = []
    for i, name in enumerate(SM.SHAPES):
        if "SOTS_SM_SEED" in os.environ:
            seeds = [int(os.environ["SOTS_SM_SEED"]) + 100 * i + j for j in range(n)]
        else:
            seeds = (SM.SEEDS[name] + [SM.SEEDS[name][-1] + 1 + j for j in range(max(0, n - 12))])[:n]
        if replay:
            seed, k = (int(x) for x in replay.split(":"))
            out += [(name, seed, k)] if seed in seeds else []
        else:
            out += [(name, s, None) for s in seeds]
    return out


REBUILD = ("set_target_audio", "set_target_spectrum", "set_objective", "set_objective_weights", "set_voice_waveforms", "set_voice_feedback")
ORDER = ("set_survivors", "set_synth_arithmetic", "set_voice_waveforms", "set_voice_feedback", "set_objective", "set_objective_weights", "target")


class FreshLandscape:
    """reference C: B's list, every landscape on a context that has seen no other"""

    def __init__(self, pkg, sh):
        self.pkg, self.sh, self.settings, self.track_args = pkg, sh, {}, None
        self.ctx = self.fresh()

    def fresh(self):
        ctx = self.sh.make(self.pkg)
        ctx.set_sort_mode(SM.SORT_FULL)
        ctx.set_select_plan(SM.PLAN_TILES)
        return ctx

    def apply(self, op):
        name = op[0]
        if name in REBUILD:
            self.settings["target" if name.startswith("set_target") else name] = op
            old = self.ctx
            v, s, f = old.read_population()
            g = old.generation
            old.close()
            self.ctx = new = self.fresh()
            for key in ORDER:
                if key in self.settings:
                    SM.apply(new, self.settings[key], self.sh)
            if self.track_args:
                new.track(*self.track_args)
            new.write_population(v, s, f)
            new.generation = g
            return None
        if name in ("set_survivors", "set_synth_arithmetic"):
            self.settings[name] = op
        if name == "track":
            self.track_args = op[1:] if (op[1] or op[2]) else None
        return SM.apply(self.ctx, op, self.sh)

    def close(self):
        self.ctx.close()


def run(pkg, shape, seed, k=None, n_ops=None):
    """None, or the text of the first mismatch"""
    sh = SM.Shape(shape)
    ops, _, boundaries = SM.generate(shape, seed, n_ops or int(os.environ.get("SOTS_SM_OPS", SM.OPS)))
    if k is not None:
        ops = SM.cut(shape, ops, boundaries, k)
    a, b = sh.make(pkg), sh.make(pkg)
    b.set_sort_mode(SM.SORT_FULL)
    b.set_select_plan(SM.PLAN_TILES)
    c = FreshLandscape(pkg, sh)
    b_ops = iter(SM.normalise(ops))
    runs_a, runs_b, runs_c = [], [], []

    def reference():
        for op in b_ops:
            r, rc = SM.apply(b, op, sh), c.apply(op)
            if op[0] == "b_until":
                runs_b.append(r)
                runs_c.append(rc)
            if op[0] in ("checkpoint", "checkpoint_all"):
                return r, rc
        raise AssertionError("B's list ended before A's checkpoint")

    try:
        checkpoint = 0
        for i, op in enumerate(ops):
            r = SM.apply(a, op, sh)
            if op[0] == "execute_until":
                runs_a.append(r)
            if op[0] not in ("checkpoint", "final_lazy"):
                continue
            got = r if op[0] == "checkpoint" else SM.snapshot(a, sh, sh.P, False, False)
            want, fresh = reference()
            got["execute_until.generations_run"] = np.array(runs_a, np.uint32)
            want["execute_until.generations_run"] = np.array(runs_b, np.uint32)
            fresh["execute_until.generations_run"] = np.array(runs_c, np.uint32)
            d, who = SM.first_difference(got, want), "B, the replay"
            if not d:
                d, who = SM.first_difference(got, fresh), "C, the replay on fresh contexts"
            if d:
                return dict(shape=shape, seed=seed, checkpoint=checkpoint, op_index=i, array=d[0], row=d[1], against=who[0],
                            text=f"{shape} seed {seed}: checkpoint {checkpoint} (call {i}) differs from {who} in {d[0]!r}, first at row {d[1]}.\n"
                                 f"Replay with SOTS_SM_REPLAY={seed}:{i + 1}.  The calls up to there (sh = SM.Shape({shape!r})):\n"
                                 + SM.listing(ops[:i + 1]))
            checkpoint += 1
        return None
    finally:
        a.close()
        b.close()
        c.close()


@pytest.mark.parametrize("shape,seed,k", cases())
def test_random_call_order_equals_its_replay(pkg, shape, seed, k):
    t = time.time()
    bad, error = None, None
    try:
        bad = run(pkg, shape, seed, k)
    except Exception as e:  # (a call that fails, a refusal that is not refused: reported, then raised)
        error = e
    if "SOTS_SM_REPORT" in os.environ:
        line = dict(shape=shape, seed=seed, seconds=round(time.time() - t, 3), ok=bad is None and error is None)
        if bad:
            line.update({x: bad[x] for x in ("checkpoint", "op_index", "array", "row", "against")})
        if error:
            line["error"] = str(error)[:300]
        with open(os.environ["SOTS_SM_REPORT"], "a") as f:
            f.write(json.dumps(line) + "\n")
    if error:
        raise error
    assert bad is None, bad["text"]
