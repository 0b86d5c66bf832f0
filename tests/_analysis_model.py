"""The fp64 model of the analysis on the device (sots_batch_analyse_audio_hop, sots_batch_queue_score_audio_hop; DESIGN.md
4.12), for the tests: frames -> window -> real DFT -> normalised magnitudes, and the score sum.

The window and the two factors come from the formulas of host/Objective_tables.hpp, restated here in NumPy:

    w[i]   = 1 - cos(i (1/N - 1) 2 pi)            in double, 1/N an fp32 number
    wf     = (sum_i w[i], accumulated in ONE fp32) * (1/N)
    m_k    = |DFT(frame * w)[k]| * fp32(1/N) * fp32(1/wf),   k = 0 .. N/2-1
    F      = sum_k w_k e_k^2,   e_k = m_k - t_k, or ln(m_k + eps) - ln(t_k + eps)
"""
import numpy as np

FFT_DELTA = 3e-6   # per-bin error of an fp32 transform, relative to the frame's largest magnitude ("Numerics")


def window(n):
    """(w[n] in double, the fp32 window factor) as sots_tables::window makes them"""
    one_over = np.float32(1.0) / np.float32(n)
    w = 1.0 - np.cos(np.arange(n, dtype=np.float64) * np.float64(one_over - np.float32(1.0)) * (2.0 * np.pi))
    f = np.float32(0.0)
    for x in w:   # f += w[i] with f an fp32: every partial sum rounded
        f = np.float32(np.float64(f) + x)
    return w, np.float32(f * one_over)


def frames(signal, n, hop, count):
    """[count][n]: frame f = signal[f hop : f hop + n], a view"""
    signal = np.ascontiguousarray(signal)
    assert signal.ndim == 1 and count >= 1 and signal.size >= (count - 1) * hop + n
    return np.lib.stride_tricks.as_strided(signal, (count, n), (hop * signal.strides[0], signal.strides[0]), writeable=False)


def magnitudes(signal, n, hop, count, win=None):
    """fp64 [count][n/2]"""
    w, wf = window(n) if win is None else win
    scale = np.float64(np.float32(1.0) / np.float32(n)) * np.float64(np.float32(1.0) / wf)
    x = frames(np.asarray(signal, np.float32), n, hop, count).astype(np.float64) * w
    return np.abs(np.fft.rfft(x, axis=-1))[:, : n // 2] * scale


def frame_count(samples, n, hop):
    return (samples - n) // hop + 1 if samples >= n else 0


def errors(m, t, eps=None):
    """e_k of magnitudes m against targets t, bin for bin: linear (eps None) or log with the floor eps"""
    m, t = np.asarray(m, np.float64), np.asarray(t, np.float64)
    if eps is None:
        return m - t
    return np.log1p((m - t) / (t + eps))   # ln(m + eps) - ln(t + eps) without the cancellation of two logarithms


def score(m, t, w=None, eps=None):
    """F per frame: m[frames][bins] against t[frames][bins], weights w[bins] or none"""
    e2 = errors(m, t, eps) ** 2
    return np.sum(e2 if w is None else np.asarray(w, np.float64) * e2, axis=-1)
