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
