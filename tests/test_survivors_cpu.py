"""CPU-side checks of elitist survival (sots_set_survivors, sots_get_survivors, sots_batch_set_survivors): the symbols are
exported, null handles are refused, and the oracle-composed elitist generation that the GPU tests compare against
(tests/_survivors_model.py) does what the rule says - on the shipped shape, whose 16 parents in a block of 32 leave
recombination with no selection pressure at all."""
import ctypes as C

import numpy as np
import pytest

from _survivors_model import PMAX, SEED, survivor_generation, survivor_variation, targets

NEW = ["sots_set_survivors", "sots_get_survivors", "sots_batch_set_survivors"]
SHIPPED = dict(kind=1, log2n=11, parents=16, offspring=16, block=32)
CHUNKS, GENERATIONS = 4, 60


def test_new_symbols_are_exported(hip):
    lib = hip.load()
    for n in NEW:
        assert n in hip.EXPORTS and hasattr(lib, n), n


def test_null_handles_are_refused(hip):
    lib = hip.load()
    n = C.c_uint32(7)
    assert lib.sots_set_survivors(None, 1) == -1
    assert "null context" in lib.sots_last_error(None).decode()
    assert lib.sots_get_survivors(None, C.byref(n)) == -1
    assert "null context" in lib.sots_last_error(None).decode()
    assert n.value == 7
    assert lib.sots_batch_set_survivors(None, 1) == -1
    assert "null batch" in lib.sots_batch_last_error(None).decode()


def oracle_es(O, chunk):
    w = SHIPPED
    ref = O.OracleES(w["parents"], w["offspring"], synth_kind=w["kind"], audio_log2=w["log2n"], param_max=PMAX[w["kind"]],
                     seed=SEED, recomb_block=w["block"])
    ref.set_target_audio(targets(CHUNKS, 1 << w["log2n"])[chunk])
    ref.init_population(chunk)
    return ref


@pytest.fixture(scope="module")
def row0(O):
    """row 0's fitness after every generation: {K: [chunk][generation]}"""
    out = {}
    for k in (0, 1):
        out[k] = []
        for chunk in range(CHUNKS):
            ref = oracle_es(O, chunk)
            out[k].append([float(survivor_generation(ref, k, g)[0]) for g in range(GENERATIONS)])
    return out


def test_with_one_survivor_row_0_never_rises(row0):
    for chunk, best in enumerate(row0[1]):
        assert all(b <= a for a, b in zip(best, best[1:])), (chunk, best)


def test_without_survivors_row_0_rises_in_every_chunk(row0):
    for chunk, best in enumerate(row0[0]):
        assert any(b > a for a, b in zip(best, best[1:])), (chunk, best)


@pytest.mark.parametrize("k", [1, 5, 16])
def test_variation_carries_rows_below_k_and_leaves_the_others_alone(O, k):
    plain, kept = oracle_es(O, 2), oracle_es(O, 2)
    for ref in (plain, kept):  # a sorted, evaluated population to start from
        survivor_generation(ref, 0, 0)
    _, _, v_plain, s_plain = survivor_variation(plain, 0, 1)
    v0, s0, v1, s1 = survivor_variation(kept, k, 1)
    hv, hs, _ = kept.read_population()  # what the oracle holds is what was returned
    assert np.array_equal(hv, v1) and np.array_equal(hs, s1)
    assert np.array_equal(v1[:k], v0[:k]) and np.array_equal(s1[:k], s0[:k])
    assert np.array_equal(v1[k:], v_plain[k:]) and np.array_equal(s1[k:], s_plain[k:])
    assert not np.array_equal(v_plain[:k], v0[:k])  # ... and without survivors those rows do change
