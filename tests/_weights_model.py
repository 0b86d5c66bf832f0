"""The fp64 model of the weighted spectral objective (sots_set_objective_weights), for the tests.

    F = sum_k w_k e_k^2,   k = 0 .. N/2-1

with e_k the signed error of the objective in force on the magnitudes of _objective_model.magnitudes: m_k - t_k under
MAGNITUDE, ln(m_k + eps) - ln(t_k + eps) under LOG_MAGNITUDE (eps given).  The device squares u_k e_k with u_k = fp32
sqrt(w_k); the model keeps w_k, and the difference (half an ulp of u_k, relative) lies inside the 1e-4 F term of the bound."""
import numpy as np

from _objective_model import FFT_DELTA, FIT_RTOL


def errors(m, t, eps=None):
    """e_k of magnitudes m[..., bins] against t[bins]: linear (eps None) or log with the floor eps"""
    m, t = np.asarray(m, np.float64), np.asarray(t, np.float64)
    if eps is None:
        return m - t
    return np.log1p((m - t) / (t + eps))  # ln(m + eps) - ln(t + eps) without the cancellation of two logarithms


def weighted_distance(m, t, w, eps=None):
    return np.sum(np.asarray(w, np.float64) * errors(m, t, eps) ** 2, axis=-1)


def tolerance(m, t, w, eps=None, lam=0.0):
    """the bound on |F_device - F_model| per row:  sum_k w_k (2 |e_k| d_k + d_k^2) + FIT_RTOL F_model, with d_k = delta under
    MAGNITUDE and delta / (m_k + eps) + lam under LOG; delta = FFT_DELTA max_k m_k over ALL bins, the masked ones
    included (the transform's error does not know the weights), lam the absolute error of the device's ln map"""
    m, t, w = np.asarray(m, np.float64), np.asarray(t, np.float64), np.asarray(w, np.float64)
    e = np.abs(errors(m, t, eps))
    delta = FFT_DELTA * np.max(m, axis=-1, keepdims=True)
    d = delta + 0.0 * m if eps is None else delta / (m + eps) + lam
    return np.sum(w * (2 * e * d + d * d), axis=-1) + FIT_RTOL * np.sum(w * e * e, axis=-1)


def fixed_weights(n, seed=0x5EED0007):
    """the GPU tests' weight vector for rows of n samples: uniform in [0, 2], a run of zeros on bins n/8 .. n/4 and a run
    of exact ones behind it (bins n/4+1 .. n/4+n/16)"""
    half = n // 2
    w = np.random.default_rng(seed).uniform(0.0, 2.0, half).astype(np.float32)
    w[n // 8:n // 4 + 1] = 0.0
    w[n // 4 + 1:n // 4 + 1 + n // 16] = 1.0
    return w

