"""Carried rows in the chunk queue (sots_batch_queue_set_carry) composed on the CPU oracle: the sequence
the header gives as the definition - inside a segment of L chunks, chunk k starts from chunk k-1's best-ever record (row 0)
and rows 1..R-1 of its last sorted population, beside the fresh rows R..P-1 of init_population(first + k) - built from the
oracle's stages and _survivors_model.survivor_generation, with the best-ever record and the stop rule kept here as k_track
and sots_stop_rule_holds keep them.  The oracle knows nothing of carrying; with R = 0, or L = 1, this is the plain chunk
sequence.

Also the gliding track the feature is for, and the per-segment sums of generations_run that the queue's makespan is made of."""
import numpy as np

from _survivors_model import survivor_generation

TURN_SECONDS = 4.0
STALL_RULE = dict(target=None, stall=50, check_every=25)   # a 50-generation stall looked at every 25 generations


def gliding_track(chunks, n=2048, hop=512, jump=False):
    """one tone gliding up an octave every 2 s, with its octave and a little noise, as a flat fp32 signal of
    (chunks - 1) hop + n samples: f(t) = 330 Hz 2^(t / 2 s), phase = 2 pi cumsum(f) / 44100,
    x = 0.6 sin(phase) + 0.3 sin(2 phase) + 0.02 default_rng(7).standard_normal.  jump: from the middle on the glide
    continues from 523 Hz instead.  A track longer than TURN_SECONDS (tools/queue_carry_bench.py's) turns there, two octaves
    up, and glides down again at the same rate instead of leaving the audible range."""
    total = (chunks - 1) * hop + n
    t = np.arange(total) / 44100.0
    up = np.abs((t + TURN_SECONDS) % (2.0 * TURN_SECONDS) - TURN_SECONDS)   # t itself up to the turn: every track of the tests
    f = 330.0 * 2.0 ** (up / 2.0)
    if jump:
        f[total // 2:] *= 523.0 / 330.0
    phase = 2.0 * np.pi * np.cumsum(f) / 44100.0
    x = 0.6 * np.sin(phase) + 0.3 * np.sin(2.0 * phase) + 0.02 * np.random.default_rng(7).standard_normal(total)
    return x.astype(np.float32)


def gliding_targets(chunks, n=2048, hop=512, jump=False):
    """chunk k = samples [k hop, k hop + n) of the gliding track: [chunks][n]"""
    x = gliding_track(chunks, n, hop, jump)
    return np.stack([x[k * hop:k * hop + n] for k in range(chunks)])


def rule_holds(rule, best_fitness, best_generation, generation):
    """sots_stop_rule_holds: a target the best-ever fitness has reached, or a stall of at least rule['stall'] generations"""
    target, stall = rule.get("target"), rule.get("stall", 0)
    if target is not None and target >= 0 and best_fitness <= np.float32(target):
        return True
    return bool(stall) and generation - best_generation >= stall


def run_chunk(ref, survivors, max_generations, rule):
    """sots_execute_until on the oracle's current population, the generation counter from 0: the first multiple of
    rule['check_every'] at which the rule holds, or max_generations.  The record is k_track's: strictly better only.
    Returns {generations_run, best_ever_generation, best_ever_fitness, best_ever_values, best_ever_steps, last_fitness,
    last_values}; the oracle holds the last sorted population."""
    best_f, best_g = np.float32(np.inf), 0
    best_v, best_s = np.zeros(ref.D, np.float32), np.zeros(ref.D, np.float32)
    run, last = 0, None
    for g in range(max_generations):
        f = survivor_generation(ref, survivors, g)
        run = g + 1
        if f[0] < best_f:
            v, s, _ = ref.read_population()
            best_f, best_g, best_v, best_s = f[0], run, v[0].copy(), s[0].copy()
        last = f[0]
        if rule is not None and run % rule["check_every"] == 0 and rule_holds(rule, best_f, best_g, run):
            break
    v, _, _ = ref.read_population()
    return dict(generations_run=run, best_ever_generation=best_g, best_ever_fitness=best_f, best_ever_values=best_v,
                best_ever_steps=best_s, last_fitness=last, last_values=v[0].copy())


def carry_sequence(ref, targets, first, survivors, carry_rows, segment_chunks, max_generations, rule):
    """the reference sequence of the header on one oracle `ref`, chunk after chunk: a list of run_chunk's results"""
    out = []
    for k, target in enumerate(targets):
        successor = carry_rows > 0 and k % segment_chunks != 0
        if successor:   # the state chunk k-1 left
            pv, ps, _ = ref.read_population()
            bv, bs = out[-1]["best_ever_values"], out[-1]["best_ever_steps"]
        ref.set_target_audio(target)
        ref.init_population(first + k)
        if successor:
            v, s, _ = ref.read_population()
            v[:carry_rows], s[:carry_rows] = pv[:carry_rows], ps[:carry_rows]
            v[0], s[0] = bv, bs
            ref.write_population(v, s, None)
        out.append(run_chunk(ref, survivors, max_generations, rule))
    return out


def track_figures(results):
    """(sum of generations_run, mean best-ever fitness, mean |difference| of the best-ever genes of neighbouring chunks)"""
    genes = np.stack([r["best_ever_values"] for r in results]).astype(np.float64)
    jumps = float(np.abs(np.diff(genes, axis=0)).mean()) if len(results) > 1 else 0.0
    return (int(sum(int(r["generations_run"]) for r in results)),
            float(np.mean([np.float64(r["best_ever_fitness"]) for r in results])), jumps)


def segment_sums(generations_run, segment_chunks):
    """generations a slot spends on each segment: a successor starts in the generation after its predecessor's last, so a
    segment is one job of the queue's in-order refill, as long as the sum of its chunks' generations_run"""
    runs = [int(g) for g in generations_run]
    return [sum(runs[i:i + segment_chunks]) for i in range(0, len(runs), segment_chunks)]
