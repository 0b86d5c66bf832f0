"""CPU-side checks of the chunks-in-flight handle (sots_batch_*): the configuration is validated before any device is
looked for, and a valid one fails with SOTS_ERR_NO_DEVICE on a machine without a gfx950 device (no CPU fallback)."""
import ctypes as C

import pytest


def _cfg(hip, **over):
    cfg = hip.make_config(16, 16, hip.SYNTH_2OP, 10, None, [3520.0, 8.0, 3520.0, 1.0], seed=1)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _create(hip, cfg, max_chunks):
    lib = hip.load()
    h = C.c_void_p()
    rc = lib.sots_batch_create(C.byref(cfg) if cfg is not None else None, max_chunks, C.byref(h))
    return rc, h


@pytest.mark.parametrize("over,max_chunks,needle", [
    (dict(), 0, "max_chunks"),
    (dict(num_parents=512, num_offspring=544), 4, "at most 1024"),           # P = 1056 > kSortSmall
    (dict(num_parents=512, num_offspring=512), (1 << 16) + 1, "2^26"),       # max_chunks x P > 2^26
    (dict(num_dimensions=6), 4, "numDimensions"),                            # 2-op voice with the 3-op D
    (dict(synth_kind=1), 4, "numDimensions"),                                # 3-op voice with the 2-op D
    (dict(struct_size=12), 4, "struct_size"),
    (dict(audio_length_log2=16), 4, "audioLengthLog2"),
    (dict(workgroup_size=24), 4, "workgroupSize"),
])
def test_batch_create_rejects_bad_configs(hip, over, max_chunks, needle):
    rc, h = _create(hip, _cfg(hip, **over), max_chunks)
    assert rc == -1 and not h.value
    assert needle in hip.load().sots_batch_last_error(None).decode()


# code and full text as the library gave them before the checks moved into csrc/sots_rules.h: one fault per call.
# SHARED: the faults the rules own, for a context and a batch alike; the rest are the batch's own limits.
SHARED = [
    (dict(struct_size=12), "sots_config.struct_size 12 != 176"),
    (dict(synth_kind=9), "unknown synth_kind 9"),
    (dict(num_dimensions=6), "synth_kind 0 needs numDimensions 4, got 6"),
    (dict(synth_kind=1), "synth_kind 1 needs numDimensions 6, got 4"),
    (dict(audio_length_log2=7), "audioLengthLog2 7 outside 8..15"),
    (dict(audio_length_log2=16), "audioLengthLog2 16 outside 8..15"),
    (dict(num_parents=0), "population 16 (parents 0) not supported"),
    (dict(num_parents=1, num_offspring=0, workgroup_size=1), "population 1 (parents 1) not supported"),
    (dict(workgroup_size=0), "populationLength 32 must be a multiple of workgroupSize 0 (the recombination block)"),
    (dict(workgroup_size=24), "populationLength 32 must be a multiple of workgroupSize 24 (the recombination block)"),
]
RECORDED_BATCH_CREATE = [(over, 4, text) for over, text in SHARED] + [
    (dict(), 0, "max_chunks must be at least 1"),
    (dict(num_parents=512, num_offspring=544), 4,
     "a batch takes chunk populations of at most 1024, got 1056 (larger ones fill the GPU alone: sots_create)"),
    (dict(num_parents=1 << 25, num_offspring=(1 << 25) + 32), 4,
     "a batch takes chunk populations of at most 1024, got 67108896 (larger ones fill the GPU alone: sots_create)"),
    (dict(num_parents=512, num_offspring=512), (1 << 16) + 1, "max_chunks 65537 x population 1024 exceeds 2^26 rows"),
]


@pytest.mark.parametrize("over,max_chunks,text", RECORDED_BATCH_CREATE)
def test_batch_create_refusals_keep_their_text(hip, over, max_chunks, text):
    rc, h = _create(hip, _cfg(hip, **over), max_chunks)
    assert rc == -1 and not h.value
    assert hip.load().sots_batch_last_error(None).decode() == text


def test_shared_faults_read_the_same_from_both_create_calls(hip):
    lib = hip.load()
    for over, text in SHARED:
        h = C.c_void_p()
        assert lib.sots_create(C.byref(_cfg(hip, **over)), C.byref(h)) == -1 and not h.value
        rc, hb = _create(hip, _cfg(hip, **over), 4)
        assert rc == -1 and not hb.value
        assert lib.sots_last_error(None).decode() == lib.sots_batch_last_error(None).decode() == text, over


@pytest.mark.parametrize("name,args", [
    ("sots_batch_set_objective", (0, 0.0)),
    ("sots_batch_set_objective_weights", (None, 0)),
    ("sots_batch_set_survivors", (0,)),
    ("sots_batch_track", (0, 0, 0)),
    ("sots_batch_set_synth_arithmetic", (0,)),
])
def test_batch_setters_refuse_a_null_batch(hip, name, args):
    lib = hip.load()
    assert getattr(lib, name)(None, *args) == -1
    assert lib.sots_batch_last_error(None).decode() == "null batch"


def test_batch_null_arguments(hip):
    lib = hip.load()
    assert lib.sots_batch_create(None, 4, None) == -1
    assert b"null" in lib.sots_batch_last_error(None)
    h = C.c_void_p()
    assert lib.sots_batch_create(C.byref(_cfg(hip)), 4, None) == -1
    assert lib.sots_batch_create(None, 4, C.byref(h)) == -1 and not h.value
    assert lib.sots_batch_execute_generations(None, 1) == -1
    assert lib.sots_batch_init_population(None, 0) == -1
    assert lib.sots_batch_read_best(None, None, 0, None, 0) == -1
    lib.sots_batch_destroy(None)  # harmless


def test_batch_limits_accept_the_largest_shapes(hip):
    """P = 1024 and max_chunks x P = 2^26 exactly are inside the limits: they fail for want of a device, not as invalid."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the GPU suite covers the success path")
    for over, chunks in ((dict(num_parents=512, num_offspring=512), 64), (dict(num_parents=32, num_offspring=32), 1 << 20)):
        rc, h = _create(hip, _cfg(hip, **over), chunks)
        assert rc == -3 and not h.value, hip.load().sots_batch_last_error(None)


def test_batch_no_cpu_fallback_without_a_gpu(hip):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; the GPU suite covers the success path")
    rc, h = _create(hip, _cfg(hip), 8)
    assert rc == -3 and not h.value
    assert "device" in hip.load().sots_batch_last_error(None).decode().lower()
    with pytest.raises(hip.SotsError):
        hip.HipBatch(8, 16, 16, hip.SYNTH_2OP, 10, None, [3520.0, 8.0, 3520.0, 1.0])
