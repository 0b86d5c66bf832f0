"""The fp64 model of the log-magnitude objective (sots_set_objective), for the tests.

NumPy on spectra from the CPU oracle (oracle.rfft / oracle.spectrum); the oracle itself knows nothing of this objective.

    F_log = sum_k (ln(m_k + eps) - ln(t_k + eps))^2,   k = 0 .. N/2-1

with m_k = |X_k| / N / windowFactor the candidate's normalised magnitude and t_k the target's - the bins and the
normalisation of the oracle's linear fitness."""
import numpy as np

FFT_DELTA = 3e-6   # per-bin error of the fp32 transform, relative to the row's largest magnitude ("Numerics")
FIT_RTOL = 1e-4    # the project's relative fitness tolerance


def magnitudes(O, audio_rows):
    """fp64 normalised magnitudes [rows][N/2] of unwindowed audio rows, through the oracle's window and fp64 transform"""
    audio_rows = np.atleast_2d(np.asarray(audio_rows, np.float32))
    n = audio_rows.shape[1]
    win, wf = O.window(n)
    out = np.empty((audio_rows.shape[0], n // 2))
    for i, a in enumerate(audio_rows):
        out[i] = np.abs(O.rfft(a, win))[: n // 2]
    return out / n / float(wf)


def log_distance(m, t, eps):
    """F_log of magnitudes m[..., bins] against t[bins]; ln(m + eps) - ln(t + eps) as log1p((m - t) / (t + eps)), the same
    number without the cancellation of two logarithms"""
    m, t = np.asarray(m, np.float64), np.asarray(t, np.float64)
    return np.sum(np.log1p((m - t) / (t + eps)) ** 2, axis=-1)


def tolerance(m, t, eps, lam):
    """the bound on |F_device - F_model| per row:  sum_k (2 |e_k| d_k + d_k^2) + FIT_RTOL F,  d_k = delta / (m_k + eps) + lam
    with delta = FFT_DELTA max_k m_k (what a magnitude error of delta does to ln(m_k + eps)) and lam the absolute error of
    the device's ln map"""
    m, t = np.asarray(m, np.float64), np.asarray(t, np.float64)
    e = np.abs(np.log1p((m - t) / (t + eps)))
    delta = FFT_DELTA * np.max(m, axis=-1, keepdims=True)
    d = delta / (m + eps) + lam
    return np.sum(2 * e * d + d * d, axis=-1) + FIT_RTOL * np.sum(e * e, axis=-1)
