"""The NumPy statement of sots_render_overlap_add, for the tests: exact, not a bound.

    acc[n] = sum  w[n - c hop] * a_c[n - c hop]     over the chunks c that cover n, ASCENDING c,
    den[n] = sum  w[n - c hop]                      same chunks, same order,
    out[n] = den[n] > 0 ? acc[n] / den[n] : 0       (samples no chunk covers are 0)

all in fp32, one multiply and then one add per term.  a_c is row c's audio from the CPU oracle (oracle.synth, or
oracle.synth_ocl for the device kernels' arithmetic), w the fp32 window table oracle.window(N)[0].astype(float32), or
all ones.  Adding whole rows in ascending c adds, at every sample, the covering chunks in ascending c: the same sums in
the same order (samples a row does not cover are not touched, so no +0 enters a sum)."""
import numpy as np


def window32(O, n):
    """the fp32 window table the contexts upload: 1 - cos, periodic, w[0] = 0, peak 2"""
    return O.window(n)[0].astype(np.float32)


def oracle_rows(O, kind, values, pmin, pmax, n, ocl=False):
    """rows[c] = the audio of values[c] (unit-range genes) on the CPU oracle"""
    values = np.asarray(values, np.float32).reshape(len(values), -1)
    if ocl:  # the arithmetic of the reference's device kernels: fused multiply-adds, the padded table
        table = np.concatenate([O.wavetable(), np.zeros(64, np.float32)])
        return np.stack([O.synth_ocl(kind, v, pmin, pmax, n, table, 1) for v in values])
    table = O.wavetable()
    return np.stack([O.synth(kind, v, pmin, pmax, n, table) for v in values])


def accumulate(rows, hop, w=None):
    """(acc, den) over the covered length (M - 1) hop + N"""
    rows = np.asarray(rows, np.float32)
    m, n = rows.shape
    w = np.ones(n, np.float32) if w is None else np.asarray(w, np.float32)
    assert w.shape == (n,) and 1 <= hop <= n
    acc = np.zeros((m - 1) * hop + n, np.float32)
    den = np.zeros_like(acc)
    for c in range(m):  # ascending c
        s = c * hop
        acc[s:s + n] = acc[s:s + n] + w * rows[c]  # fp32 product, then fp32 sum
        den[s:s + n] = den[s:s + n] + w
    return acc, den


def overlap_add(rows, hop, w=None, out_samples=None):
    """out[out_samples] (default: the covered length): truncated when shorter, zeros behind the covered range"""
    acc, den = accumulate(rows, hop, w)
    covered = np.zeros_like(acc)
    pos = den > 0
    covered[pos] = acc[pos] / den[pos]  # fp32 / fp32: correctly rounded
    if out_samples is None:
        return covered
    out = np.zeros(out_samples, np.float32)
    k = min(out_samples, len(covered))
    out[:k] = covered[:k]
    return out


def unit_rows(m, d, seed):
    """m rows of unit-range genes in [0.05, 0.95): every voice audible, nothing at a bound"""
    return np.random.default_rng(seed).uniform(0.05, 0.95, (m, d)).astype(np.float32)


def quantise_24bit(x):
    """host/Wav_IO.hpp's writer and reader in one: a float sample as it comes back from a 24-bit PCM file"""
    scaled = np.asarray(x, np.float32) * np.float32(8388608.0)  # exact: a power of two
    q = np.trunc(scaled.astype(np.float64))  # truncation towards zero, clamped to the 24-bit range (NaN: the low end)
    q = np.where(scaled >= 8388607.0, 8388607.0, q)
    q = np.where(scaled > -8388608.0, q, -8388608.0)
    return (q / 8388608.0).astype(np.float32)  # the reader: the integer over 2^23, exact in fp32
