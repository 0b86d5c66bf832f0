"""CPU-side checks of the run record (best-ever individual, history, stop rules): the symbols are exported, null handles
are refused, the record structure has the header's layout, and sots_stop_rule_holds - pure host code - agrees with a
ten-line Python model of include/sots_hip.h's rule."""
import ctypes as C
import itertools

import numpy as np
import pytest

NEW = ["sots_track", "sots_read_best_ever", "sots_read_history", "sots_stop_rule_holds", "sots_execute_until",
       "sots_batch_track", "sots_batch_read_best_ever", "sots_batch_read_history", "sots_batch_execute_until"]


def test_new_symbols_are_exported(hip):
    lib = hip.load()
    for n in NEW:
        assert n in hip.EXPORTS and hasattr(lib, n), n


def test_null_handles_are_refused(hip):
    lib = hip.load()
    rule = hip.make_stop_rule(target=1.0, stall=3, check_every=4)
    n, t, f, g = C.c_uint32(), C.c_uint64(), C.c_float(), C.c_uint32()
    assert lib.sots_track(None, 1, 0, 0) == -1
    assert lib.sots_read_best_ever(None, None, 0, None, 0, C.byref(f), C.byref(g)) == -1
    assert lib.sots_read_history(None, None, 0, C.byref(n), C.byref(t)) == -1
    assert lib.sots_execute_until(None, 10, C.byref(rule), C.byref(n)) == -1
    assert lib.sots_batch_track(None, 1, 0, 0) == -1
    assert lib.sots_batch_read_best_ever(None, None, 0, None, 0, None, 0, None, 0) == -1
    assert lib.sots_batch_read_history(None, 0, None, 0, C.byref(n), C.byref(t)) == -1
    assert lib.sots_batch_execute_until(None, 10, C.byref(rule), C.byref(n)) == -1


def test_record_layouts(hip):
    assert C.sizeof(hip.GenRecord) == 96
    assert hip.GEN_RECORD_DTYPE.itemsize == 96
    assert hip.GenRecord.mean_step.offset == 32 and hip.GEN_RECORD_DTYPE.fields["mean_step"][1] == 32
    assert hip.GenRecord.parent_mean_fitness.offset == 16
    assert C.sizeof(hip.StopRule) == 16


def model_holds(target, stall, best_ever_fitness, best_ever_generation, generation):
    """the rule of include/sots_hip.h: a fitness target (negative = off), a stall (0 = off, saturating difference)"""
    if target >= 0 and best_ever_fitness <= target:
        return 1
    if stall != 0 and max(0, generation - best_ever_generation) >= stall:
        return 1
    return 0


FITNESS = [0.0, 0.25, 0.5, 1.0, 3.0e4, float("inf"), float("nan")]
GENERATIONS = [0, 1, 7, 8, 9, 100, 2**32 - 1]


@pytest.mark.parametrize("target", [-1.0, 0.0, 0.5, 1.0e9])
@pytest.mark.parametrize("stall", [0, 1, 8, 2**31])
def test_stop_rule_agrees_with_the_model(hip, target, stall):
    lib = hip.load()
    for interval in (1, 32):
        rule = hip.make_stop_rule(target=target, stall=stall, check_every=interval)
        for f, bg, g in itertools.product(FITNESS, GENERATIONS, GENERATIONS):
            f32 = float(np.float32(f))
            got = lib.sots_stop_rule_holds(C.byref(rule), f32, bg, g)
            assert got == model_holds(target, stall, f32, bg, g), (target, stall, f, bg, g)
    if target < 0 and stall == 0:  # both conditions off: never holds
        rule = hip.make_stop_rule(target=None, stall=0, check_every=1)
        assert all(lib.sots_stop_rule_holds(C.byref(rule), 0.0, 0, g) == 0 for g in GENERATIONS)


def test_stop_rule_rejects_bad_rules(hip):
    lib = hip.load()
    assert lib.sots_stop_rule_holds(None, 0.0, 0, 0) == -1
    rule = hip.make_stop_rule(target=1.0, stall=1, check_every=0)  # check_interval 0
    assert lib.sots_stop_rule_holds(C.byref(rule), 0.0, 0, 10) == -1
    rule = hip.make_stop_rule(target=1.0, stall=1, check_every=4)
    rule.struct_size = 12
    assert lib.sots_stop_rule_holds(C.byref(rule), 0.0, 0, 10) == -1
    rule.struct_size = C.sizeof(hip.StopRule)
    assert lib.sots_stop_rule_holds(C.byref(rule), 0.0, 0, 10) == 1
