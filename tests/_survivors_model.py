"""The elitist generation (sots_set_survivors) composed on the CPU oracle from the stages it already exposes: read the
sorted population, recombine(), mutate(), write rows 0..K-1 back as they were before variation, evaluate(), sort().
The oracle itself knows nothing of survivors; with K = 0 this is its own generation.

Also the noisy targets of the shipped workload (the recipe of tools/track_overhead.py:targets, restated here so that the
CPU tests do not import a GPU tool)."""
import numpy as np

PMAX = {0: [3520.0, 8.0, 3520.0, 1.0],
        1: [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0],
        2: [3520.0, 8.0, 3520.0, 1.0] + [0.0] * 8,
        3: [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0]}
SEED = 0x5EED0001


def targets(chunks, n):
    t = np.arange(n) / 44100.0
    out = np.empty((chunks, n), np.float32)
    for c in range(chunks):
        rng = np.random.default_rng(c)
        f = 110.0 * (1 + c % 13)
        out[c] = (0.6 * np.sin(2 * np.pi * f * t) + 0.3 * np.sin(2 * np.pi * 2.7 * f * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return out


def survivor_variation(ref, k, generation):
    """recombine + mutate of the oracle's current (sorted) population under Philox generation counter `generation`, rows
    0..k-1 then restored.  Returns (sorted values, sorted steps, varied values, varied steps); the oracle holds the varied
    population."""
    ref.set_generation(generation)
    v0, s0, _ = ref.read_population()
    ref.recombine()
    ref.mutate()
    v1, s1, _ = ref.read_population()
    if k:
        v1[:k] = v0[:k]
        s1[:k] = s0[:k]
        ref.write_population(v1, s1, None)
    return v0, s0, v1, s1


def survivor_generation(ref, k, generation):
    """one elitist generation on the oracle; returns the sorted fitness"""
    survivor_variation(ref, k, generation)
    ref.evaluate()
    ref.sort()
    return ref.read_population()[2]
