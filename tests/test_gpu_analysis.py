"""Analysis on the device (sots_batch_set_analysis, sots_batch_analyse_audio_hop, sots_batch_queue_score_audio_hop; DESIGN.md
4.12): the magnitudes of overlapping frames from one upload against the fp64 model of tests/_analysis_model.py, the
independence of a frame from everything but its own samples (exact bits), the audio target calls under
SOTS_ANALYSIS_DEVICE against their spectra forms fed the device's own magnitudes (exact bits), the per-chunk score, and
the refusals.

The bound of the accuracy tests is the project's bound for an fp32 transform against fp64: per frame
|device - model| <= 3e-6 max_k m_k.  The score is held to the fitness tolerance of tests/test_gpu_parity.py."""
import ctypes as C

import numpy as np
import pytest

import _analysis_model as A
from _carry_model import gliding_track
from _weights_model import fixed_weights

pytestmark = pytest.mark.gpu

PMAX = {0: [3520.0, 8.0, 3520.0, 1.0],
        1: [3520.0, 8.0, 3520.0, 8.0, 3520.0, 8.0]}
SEED = 0x5EED0001
# (voice, log2 N, parents, offspring, recombination block): the shapes of tests/test_gpu_queue_carry.py
SHIPPED = (1, 11, 16, 16, 32)
SHORT = (0, 8, 16, 16, 32)
FIT_RTOL, FIT_ATOL_REL = 1e-4, 1e-9   # tests/test_gpu_parity.py
LOG_FLOOR = 1e-3
NOT_TINY = 1e-3                       # a frame's largest bin in the accuracy tests (signals of amplitude 0.25 .. 1)
INVALID, SIZE, STATE = -1, -4, -5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def make_batch(pkg, shape, slots=4, track=True):
    kind, log2n, parents, offspring, wg = shape
    b = pkg.HipBatch(slots, parents, offspring, synth_kind=kind, audio_log2=log2n, param_max=PMAX[kind], seed=SEED, workgroup_size=wg)
    if track:
        b.track()
    return b


def band_weights(n):
    """bins n/16 .. n/4 count, the rest do not"""
    w = np.zeros(n // 2, np.float32)
    w[n // 16:n // 4] = 1.0
    return w


def chirp(total):
    """a linear chirp from 0.01 to 0.2 cycles per sample: every frame has another spectrum"""
    t = np.arange(total, dtype=np.float64)
    return (0.8 * np.sin(2.0 * np.pi * (0.01 * t + 0.5 * (0.19 / total) * t * t))).astype(np.float32)


def signals(n, hop, frames):
    """name -> signal: the FM track, the same plus noise at -40 dB, a unit impulse on the quiet track
    at sample 0 of the last frame, at N-1 of frame 0 and just past the last frame's end, and the chirp"""
    need = (frames - 1) * hop + n
    fm = gliding_track(frames, n, hop)
    rms = float(np.sqrt(np.mean(fm.astype(np.float64) ** 2)))
    noisy = (fm + 0.01 * rms * np.random.default_rng(11).standard_normal(need)).astype(np.float32)
    quiet = (0.25 * fm).astype(np.float32)
    first, last = quiet.copy(), quiet.copy()
    first[(frames - 1) * hop] += 1.0
    last[n - 1] += 1.0
    past = np.concatenate([quiet, np.ones(1, np.float32)])
    return {"fm": fm, "fm_noise": noisy, "impulse_first": first, "impulse_last": last, "impulse_past": past, "chirp": chirp(need)}


# ---- accuracy ----
@pytest.mark.parametrize("log2n", [8, 9, 10, 11, 12, 13, 14, 15])   # every instantiation of k_analyse
def test_magnitudes_against_fp64_model(pkg, log2n):
    n = 1 << log2n
    b = make_batch(pkg, (0, log2n, 16, 16, 32), slots=1, track=False)
    win = A.window(n)
    worst = 0.0
    for frames in ((7,) if log2n == 15 else (1, 7, 70)):
        for hop in (n, n // 4, 101, 1):
            for name, x in signals(n, hop, frames).items():
                want = A.magnitudes(x, n, hop, frames, win)
                peak = want.max(axis=1)
                assert peak.min() >= NOT_TINY, (name, frames, hop, peak.min())   # (on the CPU: the bound below is not vacuous)
                got = b.analyse_audio_hop(x, hop, frames)
                assert got.shape == (frames, n // 2) and got.dtype == np.float32
                err = np.abs(got.astype(np.float64) - want).max(axis=1) / peak
                worst = max(worst, float(err.max()))
                assert err.max() <= A.FFT_DELTA, (name, frames, hop, int(err.argmax()), float(err.max()))
                if name == "impulse_past":   # the sample behind the last frame is not looked at
                    assert same_bits(got, b.analyse_audio_hop(x[:-1], hop, frames))
    print(f"log2n {log2n}: worst |device - model| / max_k m_k = {worst:.3g}")
    b.close()


# ---- independence, exact bits ----
@pytest.mark.parametrize("log2n", [8, 11])
@pytest.mark.parametrize("hop", [101, 1])
def test_frame_depends_on_its_samples_only(pkg, log2n, hop):
    n, frames = 1 << log2n, 70
    b = make_batch(pkg, (0, log2n, 16, 16, 32), slots=1, track=False)
    x = gliding_track(frames, n, hop)
    whole = b.analyse_audio_hop(x, hop, frames)
    assert same_bits(whole, b.analyse_audio_hop(x, hop, frames))   # the same call twice
    for f in range(frames):
        one = b.analyse_audio_hop(x[f * hop:f * hop + n], hop, 1)
        assert same_bits(one[0], whole[f]), f
    # a frame at another hop and another place in the buffer, the same samples: the same bits
    other = b.analyse_audio_hop(x, n // 4, A.frame_count(x.size, n, n // 4))
    for f in range(0, frames, 7):
        if (f * hop) % (n // 4) == 0:
            assert same_bits(other[f * hop // (n // 4)], whole[f]), f
    b.close()


@pytest.mark.parametrize("log2n,hop", [(8, 101), (10, 256), (11, 1)])
def test_nan_poisons_the_frames_that_cover_it(pkg, log2n, hop):
    n, frames = 1 << log2n, 70
    b = make_batch(pkg, (0, log2n, 16, 16, 32), slots=1, track=False)
    x = gliding_track(frames, n, hop)
    clean = b.analyse_audio_hop(x, hop, frames)
    assert np.isfinite(clean).all()
    for at, value in ((0, np.nan), (x.size // 2, np.nan), (x.size - 1, np.inf)):
        y = x.copy()
        y[at] = value
        got = b.analyse_audio_hop(y, hop, frames)
        covered = np.array([f * hop <= at < f * hop + n for f in range(frames)])
        assert covered.any()
        assert not np.isfinite(got[covered]).any()          # every bin of a covering frame
        assert same_bits(got[~covered], clean[~covered])    # and nothing else
    b.close()


# ---- the mode ----
def objective_cases(n):
    return {"magnitude": (0, 0.0, None), "log": (1, LOG_FLOOR, None), "magnitude_weights": (0, 0.0, fixed_weights(n)),
            "log_weights": (1, LOG_FLOOR, fixed_weights(n))}


def apply_objective(b, case):
    objective, floor, w = case
    b.set_objective(objective, floor)
    b.set_objective_weights(w)


@pytest.mark.parametrize("shape", [SHIPPED, SHORT], ids=["shipped", "short"])
@pytest.mark.parametrize("case", ["magnitude", "log", "magnitude_weights", "log_weights"])
def test_device_mode_queue_equals_spectra_form(pkg, shape, case):
    n, chunks = 1 << shape[1], 8
    hop = n // 4
    x = gliding_track(chunks, n, hop)
    dev, ref = make_batch(pkg, shape), make_batch(pkg, shape)
    for b in (dev, ref):
        apply_objective(b, objective_cases(n)[case])
    dev.set_analysis(pkg.capi.ANALYSIS_DEVICE)
    dev.queue_targets_audio(x, hop)
    ref.queue_targets_spectra(ref.analyse_audio_hop(x, hop, chunks))
    got, _ = dev.queue_run(0, 50)
    want, _ = ref.queue_run(0, 50)
    assert got.size == chunks and got.tobytes() == want.tobytes()
    assert np.isfinite(got["best_ever_fitness"]).all()
    dev.close(), ref.close()


@pytest.mark.parametrize("shape", [SHIPPED, SHORT], ids=["shipped", "short"])
@pytest.mark.parametrize("case", ["magnitude", "log_weights"])
def test_device_mode_targets_equal_spectra_form(pkg, shape, case):
    n, chunks = 1 << shape[1], 4
    hop = n // 4
    x = gliding_track(chunks, n, hop)
    dev, ref = make_batch(pkg, shape), make_batch(pkg, shape)
    for b in (dev, ref):
        apply_objective(b, objective_cases(n)[case])
    dev.set_analysis(pkg.capi.ANALYSIS_DEVICE)
    dev.set_target_audio(x, hop)
    ref.set_target_spectra(ref.analyse_audio_hop(x, hop, chunks))
    for b in (dev, ref):
        b.init_population(0)
        b.execute_generations(20)
    (gv, gf), (wv, wf) = dev.read_best(), ref.read_best()
    assert same_bits(gv, wv) and same_bits(gf, wf) and np.isfinite(gf).all()
    # the hop = N form goes the same way
    y = x[:(x.size // n) * n]
    dev.set_target_audio(y.reshape(-1, n))
    ref.set_target_spectra(ref.analyse_audio_hop(y, n, y.size // n))
    for b in (dev, ref):
        b.init_population(3)
        b.execute_generations(5)
    (gv, gf), (wv, wf) = dev.read_best(), ref.read_best()
    assert same_bits(gv, wv) and same_bits(gf, wf)
    dev.close(), ref.close()


def test_mode_setting(pkg):
    shape = SHORT
    n, chunks = 1 << shape[1], 4
    hop = n // 4
    x = gliding_track(chunks, n, hop)
    b, fresh = make_batch(pkg, shape), make_batch(pkg, shape)
    assert b.get_analysis() == pkg.capi.ANALYSIS_HOST
    b.set_analysis(pkg.capi.ANALYSIS_DEVICE)
    assert b.get_analysis() == pkg.capi.ANALYSIS_DEVICE
    with pytest.raises(pkg.capi.SotsError) as e:
        b.set_analysis(2)
    assert e.value.code == INVALID and "unknown analysis mode 2" in str(e.value)
    assert b.get_analysis() == pkg.capi.ANALYSIS_DEVICE   # the old setting stays

    def run(batch, queue):
        if queue:
            batch.queue_targets_audio(x, hop)
            return batch.queue_run(0, 10)[0].tobytes()
        batch.set_target_audio(x, hop)
        batch.init_population(0)
        batch.execute_generations(10)
        v, f = batch.read_best()
        return v.tobytes() + f.tobytes()

    device_bits = run(b, False), run(b, True)
    b.set_analysis(pkg.capi.ANALYSIS_HOST)
    assert b.get_analysis() == pkg.capi.ANALYSIS_HOST
    host_bits = run(b, False), run(b, True)
    assert host_bits == (run(fresh, False), run(fresh, True))   # back on the host: a fresh default batch's bits
    assert host_bits != device_bits                             # (fp32 against fp64: the mode is not a no-op)
    b.close(), fresh.close()


# ---- score ----
@pytest.mark.parametrize("log2n", [8, 9, 10, 11, 12, 13, 14, 15])   # every instantiation of k_analyse's bins form
def test_score_of_the_target_signal_is_zero(pkg, log2n):
    n, chunks = 1 << log2n, 8
    b = make_batch(pkg, (0, log2n, 16, 16, 32))
    b.set_analysis(pkg.capi.ANALYSIS_DEVICE)
    for hop in (n // 4, 101, n):
        x = gliding_track(chunks, n, hop)
        for objective, floor, w in ((0, 0.0, None), (1, LOG_FLOOR, None), (0, 0.0, band_weights(n)), (1, LOG_FLOOR, band_weights(n))):
            b.set_objective(objective, floor)
            b.set_objective_weights(w)
            b.queue_targets_audio(x, hop)
            f = b.queue_score_audio_hop(x, hop)
            assert f.shape == (chunks,) and same_bits(f, np.zeros(chunks, np.float32)), (hop, objective, w is not None, f)
    b.close()


@pytest.mark.parametrize("shape", [SHIPPED, SHORT, (0, 12, 16, 16, 32), (0, 15, 16, 16, 32)], ids=["shipped", "short", "n4096", "n32768"])
def test_score_of_another_signal_against_the_model(pkg, shape):
    n, chunks = 1 << shape[1], 8
    hop = n // 4
    x, y = gliding_track(chunks, n, hop), gliding_track(chunks, n, hop, jump=True)
    y = (0.7 * y).astype(np.float32)
    b = make_batch(pkg, shape)
    b.set_analysis(pkg.capi.ANALYSIS_DEVICE)
    t = b.analyse_audio_hop(x, hop, chunks).astype(np.float64)   # what the queue stores under DEVICE (test_device_mode_*)
    m = b.analyse_audio_hop(y, hop, chunks).astype(np.float64)
    atol = FIT_ATOL_REL * np.sum(t * t, axis=1) + 1e-12
    for objective, floor, w in ((0, 0.0, None), (1, LOG_FLOOR, None), (0, 0.0, fixed_weights(n)), (1, LOG_FLOOR, fixed_weights(n))):
        b.set_objective(objective, floor)
        b.set_objective_weights(w)
        b.queue_targets_audio(x, hop)
        got = b.queue_score_audio_hop(y, hop).astype(np.float64)
        assert same_bits(got, b.queue_score_audio_hop(y, hop))   # a fixed order of summation
        want = A.score(m, t, w, floor if objective else None)
        assert (want > 0).all()
        assert (np.abs(got - want) <= FIT_RTOL * want + atol).all(), (objective, w is not None, got, want)
    b.close()


@pytest.mark.parametrize("shape", [SHIPPED, SHORT], ids=["shipped", "short"])
def test_score_pairs_frame_k_with_target_k(pkg, shape):
    n, chunks = 1 << shape[1], 8
    x = chirp(chunks * n)
    rev = np.ascontiguousarray(x.reshape(chunks, n)[::-1]).reshape(-1)   # the chunks in reverse order (hop = N: no overlap)
    b = make_batch(pkg, shape)
    b.set_analysis(pkg.capi.ANALYSIS_DEVICE)
    b.queue_targets_audio(x, n)
    assert same_bits(b.queue_score_audio_hop(x, n), np.zeros(chunks, np.float32))
    got = b.queue_score_audio_hop(rev, n).astype(np.float64)
    t = b.analyse_audio_hop(x, n, chunks).astype(np.float64)
    want = A.score(t[::-1], t)   # frame k of `rev` is chunk chunks-1-k, scored against target k
    assert (want > 1e-6).all() and (got > 0).all()
    assert (np.abs(got - want) <= FIT_RTOL * want + FIT_ATOL_REL * np.sum(t * t, axis=1) + 1e-12).all(), (got, want)
    b.close()


# ---- nothing disturbed ----
def test_analysis_and_score_disturb_nothing(pkg):
    shape = SHIPPED
    n, chunks = 1 << shape[1], 4
    hop = n // 4
    x = gliding_track(chunks, n, hop)
    other = gliding_track(6, n, 101, jump=True)
    a, b = make_batch(pkg, shape), make_batch(pkg, shape)
    for batch in (a, b):
        batch.queue_targets_audio(x, hop)
        batch.set_target_audio(x, hop)
        batch.init_population(0)
    a.execute_generations(10)
    a.analyse_audio_hop(other, 101)
    a.queue_score_audio_hop(x, hop)
    a.execute_generations(10)
    b.execute_generations(20)
    for c in range(chunks):
        for p, q in zip(a.read_population(c), b.read_population(c)):
            assert same_bits(p, q), c
    for p, q in zip(a.best_ever(), b.best_ever()):
        assert np.array_equal(np.ascontiguousarray(p).view(np.uint32), np.ascontiguousarray(q).view(np.uint32))
    for p, q in zip(a.read_best(), b.read_best()):
        assert same_bits(p, q)
    assert a.queue_run(0, 10)[0].tobytes() == b.queue_run(0, 10)[0].tobytes()   # the stored queue too
    a.close(), b.close()


# ---- refusals ----
def test_refusals_leave_the_state_alone(pkg):
    shape = SHORT
    n, chunks = 1 << shape[1], 4
    hop = n // 4
    x = gliding_track(chunks, n, hop)
    b = make_batch(pkg, shape)
    L, h = b.L, b._h
    p = x.ctypes.data_as(C.c_void_p)
    mags = np.full((chunks, n // 2), -7.0, np.float32)
    fit = np.full(chunks, -7.0, np.float32)
    mp, fp = mags.ctypes.data_as(C.c_void_p), fit.ctypes.data_as(C.c_void_p)
    bins = chunks * (n // 2)

    def refused(rc, code, text):
        assert rc == code, (rc, L.sots_batch_last_error(h).decode())
        assert text in L.sots_batch_last_error(h).decode(), L.sots_batch_last_error(h).decode()

    # the score before any queue is stored
    refused(L.sots_batch_queue_score_audio_hop(h, p, x.size, hop, fp, chunks), STATE, "no queue")
    b.set_analysis(pkg.capi.ANALYSIS_DEVICE)
    b.queue_targets_audio(x, hop)
    before = b.queue_score_audio_hop(0.5 * x, hop)
    analyse, score = L.sots_batch_analyse_audio_hop, L.sots_batch_queue_score_audio_hop
    # sots_batch_analyse_audio_hop
    refused(analyse(None, p, x.size, hop, chunks, mp, bins), INVALID, "")
    refused(analyse(h, None, x.size, hop, chunks, mp, bins), INVALID, "null pointer")
    refused(analyse(h, p, x.size, hop, chunks, None, bins), INVALID, "null pointer")
    refused(analyse(h, p, x.size, 0, chunks, mp, bins), INVALID, f"hop 0 outside 1..{n}")
    refused(analyse(h, p, x.size, n + 1, chunks, mp, bins), INVALID, f"hop {n + 1} outside 1..{n}")
    refused(analyse(h, p, x.size, hop, 0, mp, 0), INVALID, "at least 1")
    refused(analyse(h, p, x.size - 1, hop, chunks, mp, bins), SIZE, f"need {x.size} samples, got {x.size - 1}")
    refused(analyse(h, p, x.size, hop, chunks, mp, bins - 1), SIZE, f"{bins} bins")
    refused(analyse(h, p, x.size, hop, chunks, mp, bins + 1), SIZE, f"{bins} bins")
    # the bounds, refused before a sample is read: 2^28 samples, 2^30 bytes of spectra
    edge = ((1 << 28) - n) // hop + 1   # the most frames at this hop
    refused(analyse(h, p, 1 << 40, hop, edge + 1, mp, (edge + 1) * (n // 2)), INVALID, "more than 268435456")
    refused(analyse(h, p, 1 << 40, 1, (1 << 23) + 1, mp, ((1 << 23) + 1) * (n // 2)), INVALID, "exceed 1073741824 bytes")
    # sots_batch_queue_score_audio_hop
    refused(score(None, p, x.size, hop, fp, chunks), INVALID, "")
    refused(score(h, None, x.size, hop, fp, chunks), INVALID, "null pointer")
    refused(score(h, p, x.size, hop, None, chunks), INVALID, "null pointer")
    refused(score(h, p, x.size, 0, fp, chunks), INVALID, "hop 0 outside")
    refused(score(h, p, x.size, n + 1, fp, chunks), INVALID, f"hop {n + 1} outside")
    refused(score(h, p, x.size, hop, fp, 0), INVALID, "at least 1")
    refused(score(h, p, x.size - 1, hop, fp, chunks), SIZE, f"need {x.size} samples")
    refused(score(h, p, x.size, hop, fp, chunks - 1), SIZE, f"the queue holds {chunks} chunks, got {chunks - 1}")
    refused(score(h, p, x.size + hop, hop, fp, chunks + 1), SIZE, f"the queue holds {chunks} chunks, got {chunks + 1}")
    refused(score(h, p, 1 << 40, hop, fp, edge + 1), INVALID, "more than 268435456")
    # the mode, and the audio target calls under DEVICE beyond one upload
    refused(L.sots_batch_set_analysis(h, 2), INVALID, "unknown analysis mode 2")
    refused(L.sots_batch_set_analysis(None, 1), INVALID, "")
    refused(L.sots_batch_get_analysis(h, None), INVALID, "null pointer")
    # nothing was written, nothing changed
    assert (mags == -7.0).all() and (fit == -7.0).all()
    assert b.get_analysis() == pkg.capi.ANALYSIS_DEVICE
    assert same_bits(before, b.queue_score_audio_hop(0.5 * x, hop))
    fresh = make_batch(pkg, shape)
    fresh.set_analysis(pkg.capi.ANALYSIS_DEVICE)
    fresh.queue_targets_audio(x, hop)
    assert b.queue_run(0, 10)[0].tobytes() == fresh.queue_run(0, 10)[0].tobytes()
    b.close(), fresh.close()
