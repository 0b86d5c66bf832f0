"""Probes for the last operation of every spectral fitness kernel: bin k of the candidate against entry k of the target
table (and of the weight table), k = 0 .. N/2-1, summed.  NumPy on the CPU oracle, like _objective_model.py.

The suite's own populations (FM voices, carriers up to 3520 Hz) leave most bins some 1e-5 of the largest: two exchanged
table entries, a bin left out or the Nyquist bin in place of DC would change no fitness by more than the tolerance, or
by a bit.  The probes are made so that every such mistake moves some row far outside its bound:

* probe rows: 2-op genes with the index gene 0 - near-pure tones - in a box whose carrier runs to 22 050 Hz (PMAX).  One
  tone every second bin, a quarter bin off centre (k + 0.25, k = 0, 2, 4, ...): the main lobe of the window is then
  asymmetric and reaches the neighbour bins, so every bin is loud in some row and no two bins are equally loud in it.
  The tone at 0.25 puts energy at DC; the last one lies at N/2 - 1.25 instead of N/2 - 1.75, near enough to the Nyquist
  bin to make it loud at every N.  Amplitudes cycle through AMPS;
  a population larger than the tone set repeats it with other amplitudes.
* three (or more) sparse targets: T_j is non-zero only on bins k = j (mod 3), 0.05 .. 0.25 there.  3 is coprime to every
  power-of-two stride, so for a pair (k, k + 2^s) one of three targets is non-zero on exactly one of the two; T_0 has a
  loud DC bin.  Sparse, because under the log objective a dense target drowns one bin's change in the sum.
* probe weights: 0.25 .. 1.75, level 0.4 / 1.0 / 1.6 by k mod 3 with a seeded jitter of +-0.15 - no two bins at a
  power-of-two distance are closer than 0.3.
* the log objective is probed with the floor LOG_FLOOR = 0.1 (with 1e-2 or 1e-4 a bin near the floor outweighs the rest).

N = 16 384 and 32 768 (a workgroup per row, "coverage, not speed") are probed on three bands only - bins 0 .. 255,
N/2 - 256 .. N/2 - 1 and 128 either side of N/4 - with the tones of those bands (384 rows) and targets that are zero
outside them: under the log objective 5461 loud target bins that no tone meets would put 0.15 into every row's bound
at N = 32 768 and hide single bins of the bands.

The bound on |F_device - F_model| of a row is the suite's form with its relative term as a parameter:

    sum_k w_k (2 |e_k| d_k + d_k^2) + r F,

d_k = delta under MAGNITUDE and delta / (m_k + eps) + LAMBDA under LOG_MAGNITUDE, delta = 3e-6 max_k m_k (DESIGN.md 3,
"Numerics"; the roundings of the magnitude itself - square root, scale: below 3e-7 m_k - count as part of it, as in
_weights_model.tolerance), LAMBDA = 2.5e-6 the absolute error of the device's ln map.

r stands for what fp32 does to e_k AFTER that: the subtraction, the product with u_k, the square, the sums.  With
u = 2^-24 (round to nearest), to first order and worst case:
  - the term: e = x - t rounds once (u, relative to e; 2 u in e^2); under weights u_k = fp32 sqrt(w_k) is off by u and
    the product e u_k rounds once (4 u in the square); the square rounds once (u).  3 u without weights, 7 u with them.
  - the sum: every term is >= 0, so a sum tree in which a term passes through at most D additions is off by at most
    D u of the exact sum.  D from the kernels' reduction orders (csrc/kernels/spectral_*.h; wave_sum: csrc/kernels/common.h):
      k_fft, k_fitness (N = 512, 1024; one wavefront, wide and list forms alike): a lane adds N/256 terms into each half
        of a 2-vector, adds the halves (1), four DPP levels inside a row of 16 lanes (4), the four row totals in turn (3):
        D = N/256 + 8, 10 and 12.
      k_fft_x, k_fitness_x (N = 256, 2048, 4096, 8192; 4 or 16 wavefronts, a row per wavefront): a lane adds its N/128
        terms in turn, then the wavefront sum (7): D = N/128 + 7, 9 .. 71.
      k_fft_big, k_fitness_big (N = 16 384, 32 768; 512 threads per row): a thread adds N/1024 terms, the wavefront sum
        (7), thread 0 the eight wavefront totals (8): D = N/1024 + 15, 31 and 47.
    (the first addition onto 0 is exact; it is counted all the same.)
relative_term() returns (term + D) u (1 + 1e-3), the last factor for the higher orders: 7.2e-7 (N = 256, no weights) .. 4.7e-6
(N = 8192, weights), all below the 2e-5 the probes were designed with.  The power test (test_spectral_probe_cpu.py) holds every
single fault below to 4 x this bound."""
from collections import namedtuple

import numpy as np

from _objective_model import FFT_DELTA, magnitudes
from _weights_model import errors, weighted_distance

LAMBDA = 2.5e-6
LOG_FLOOR = 0.1
OBJECTIVES = (None, LOG_FLOOR)                  # None: MAGNITUDE; a number: LOG_MAGNITUDE with that floor
PMAX = [3520.0, 8.0, 22050.0, 1.0]              # modulator, index, carrier, amplitude
TONE_PMAX = [3520.0, 0.0, 22050.0, 1.0]         # a box in which every individual is a tone (batches draw their own rows)
AMPS = (1.0, 0.7, 0.85, 0.55)
STEP = 1e-6
U = 2.0 ** -24
POWER = 4.0                                     # a fault must move a row by this many bounds
BAND_FROM = 14                                  # log2 N from which only the bands are probed
TARGET_SEED, WEIGHT_SEED = 0x5EED0017, 0x5EED0018


# ---- the relative term ---------------------------------------------------------------------------------------------------
def sum_depth(log2n):
    n = 1 << log2n
    if log2n in (9, 10):
        return n // 256 + 8
    if log2n in (8, 11, 12, 13):
        return n // 128 + 7
    if log2n in (14, 15):
        return n // 1024 + 15
    raise ValueError(f"no spectral kernel for N = 2^{log2n}")


def relative_term(log2n, weighted):
    return ((7 if weighted else 3) + sum_depth(log2n)) * U * (1 + 1e-3)


# ---- probe rows ----------------------------------------------------------------------------------------------------------
def probed_bins(n):
    """the bins the probes answer for: all of them, or the three bands"""
    half = n // 2
    if n < 1 << BAND_FROM:
        return np.arange(half)
    return np.concatenate([np.arange(256), np.arange(n // 4 - 128, n // 4 + 128), np.arange(half - 256, half)])


def tone_bins(n):
    """the tone set: every second probed bin (the tone lies a quarter bin above it)"""
    b = probed_bins(n)
    return b[b % 2 == 0]


def probe_rows(n, rows=None):
    """(values[rows][4], steps[rows][4]) of the 2-op voice in the box PMAX: row i is the tone of tone_bins(n)[i mod T],
    amplitudes from AMPS in the first pass through the set and other ones in every further pass"""
    ks = tone_bins(n)
    rows = ks.size if rows is None else rows
    i = np.arange(rows)
    rep = i // ks.size
    amp = np.where(rep == 0, np.asarray(AMPS)[i % len(AMPS)], 0.5 + 0.5 * np.mod((i % len(AMPS)) / len(AMPS) + rep * 0.6180339887, 1.0))
    v = np.zeros((rows, 4), np.float32)
    k = ks[i % ks.size]
    v[:, 2] = (k + np.where(k == n // 2 - 2, 0.75, 0.25)) * 2.0 / n   # carrier (k + 0.25) 44100 / N Hz of 22 050
    v[:, 3] = amp
    return v, np.full((rows, 4), STEP, np.float32)


def sparse_targets(n, count=3):
    """T_j[N/2], j < count: non-zero on the probed bins k = j (mod 3) only, seeded values in 0.05 .. 0.25 (j >= 3: the
    residues again, other values)"""
    half = n // 2
    t = np.zeros((count, half), np.float32)
    for j in range(count):
        idx = probed_bins(n)
        idx = idx[idx % 3 == j % 3]
        t[j, idx] = np.random.default_rng(TARGET_SEED + j).uniform(0.05, 0.25, idx.size)
    return t


def probe_weights(n):
    half = n // 2
    k = np.arange(half)
    w = np.asarray([0.4, 1.0, 1.6])[k % 3] + np.random.default_rng(WEIGHT_SEED).uniform(-0.15, 0.15, half)
    return w.astype(np.float32)


def synthesise(O, values, n, pmax=PMAX):
    """the oracle's audio of rows of genes in a box 0 .. pmax (bit-exact with the device's)"""
    table = O.wavetable()
    return np.stack([O.synth(0, v, [0.0] * 4, pmax, n, table) for v in np.atleast_2d(values)])


def nyquist_magnitude(O, audio_rows):
    """normalised magnitude of bin N/2, which `magnitudes` leaves out: |sum_i (-1)^i a_i win_i| / N / windowFactor"""
    a = np.atleast_2d(np.asarray(audio_rows, np.float32)).astype(np.float64)
    n = a.shape[1]
    win, wf = O.window(n)
    return np.abs((a * win) @ np.where(np.arange(n) % 2, -1.0, 1.0)) / n / float(wf)


# ---- fitness and bound ---------------------------------------------------------------------------------------------------
def fitness(m, t, w=None, eps=None):
    w = np.ones(np.shape(t)[-1]) if w is None else w
    return weighted_distance(m, t, w, eps)


def per_bin_slack(m, eps=None):
    """d_k of _weights_model.tolerance"""
    m = np.asarray(m, np.float64)
    delta = FFT_DELTA * np.max(m, axis=-1, keepdims=True)
    return delta + 0.0 * m if eps is None else delta / (m + eps) + LAMBDA


def bound(m, t, w, eps, r):
    m, t = np.asarray(m, np.float64), np.asarray(t, np.float64)
    w = np.ones(t.shape[-1]) if w is None else np.asarray(w, np.float64)
    e = np.abs(errors(m, t, eps))
    d = per_bin_slack(m, eps)
    return np.sum(w * (2 * e * d + d * d), axis=-1) + r * np.sum(w * e * e, axis=-1)


def judge(f_dev, m, t, w, eps, r):
    """(|F_dev - F_model| / bound per row, F_model)"""
    want = fitness(m, t, w, eps)
    return np.abs(np.asarray(f_dev, np.float64) - want) / bound(m, t, w, eps, r), want


# ---- single faults -------------------------------------------------------------------------------------------------------
# The sum as a list of slots: slot i adds count[i] w[wi[i]] e(m[mi[i]], t[ti[i]])^2, over magnitudes with the Nyquist bin
# appended (index N/2) and tables with one entry appended (target 0, weight 1: what a table has behind its end).  The
# sound pairing is mi = ti = wi = 0 .. N/2-1, count 1; a fault is a function that changes it.
Pairing = namedtuple("Pairing", "mi ti wi count")


def sound(half):
    k = np.arange(half)
    return Pairing(k.copy(), k.copy(), k.copy(), np.ones(half))


def left_out(k):                                            # (a)
    def f(p):
        p.count[k] = 0.0
    return f


def counted_twice(k):                                       # (b)
    def f(p):
        p.count[k] = 2.0
    return f


def targets_exchanged(k, k2):                               # (c)
    def f(p):
        p.ti[k], p.ti[k2] = k2, k
    return f


def weights_exchanged(k, k2):                               # (d)
    def f(p):
        p.wi[k], p.wi[k2] = k2, k
    return f


def nyquist_added(half):                                    # (e) a slot more: bin N/2 against what lies behind the tables
    def f(p):
        return Pairing(np.append(p.mi, half), np.append(p.ti, half), np.append(p.wi, half), np.append(p.count, 1.0))
    return f


def nyquist_in_place_of(k, half):                           # (e) bin N/2 where bin k belongs: k = 0, and k = N/4, the
    def f(p):                                               #     partner of bin 0 in the pairs (k, N/2 - k) of k_fft
        p.mi[k] = half
    return f


def faulty_fitness(fault, m_ext, t, w=None, eps=None):
    """F of rows m_ext[rows][N/2 + 1] (the Nyquist bin last) under the pairing `fault` leaves (None: the sound one)"""
    half = np.shape(t)[-1]
    t_ext = np.append(np.asarray(t, np.float64), 0.0)
    w_ext = np.append(np.ones(half) if w is None else np.asarray(w, np.float64), 1.0)
    p = sound(half)
    if fault is not None:
        p = fault(p) or p
    m_ext = np.atleast_2d(m_ext)
    return np.sum(p.count * w_ext[p.wi] * errors(m_ext[:, p.mi], t_ext[p.ti], eps) ** 2, axis=-1)


def other_chunks_table(tables, c2):                         # (f) chunk c judged against chunk c2's table
    return np.asarray(tables)[c2]


def table_read_late(tables, c):                             # (g) chunk c's table read c entries late: the stride of the
    flat = np.asarray(tables).reshape(-1)                   #     image one entry short
    half = np.shape(tables)[-1]
    return flat[c * half - c:c * half - c + half]


def x_image_bins(n):
    """bin of entry (lane l, register r) of k_fft_x's target table, [64][N/128] (x_target_bin, csrc/kernels/spectral_x.h): the
    lane's own bin bitrev(r) + E bitrev6(l) for the first register of a pair (r, bitrev(E - bitrev(r))), its partner
    lane's bin for the second"""
    e = n // 128
    eb = e.bit_length() - 1

    def rev(v, width):
        return sum(((v >> i) & 1) << (width - 1 - i) for i in range(width))
    q = np.array([rev(r, eb) for r in range(e)])
    r2 = np.array([0 if x == 0 else rev(e - x, eb) for x in q])
    pp = np.array([rev(l, 6) for l in range(64)])[:, None]
    return np.where(r2 < np.arange(e), q + e * (63 - pp), q + e * pp)


def x_table_read_late(tables, c):                           # (g) in the layout of k_fft_x's segmented image: a lane's
    tables = np.asarray(tables)                             #     entries E + 4 floats apart, the last four unused (0)
    n = 2 * tables.shape[-1]
    bins = x_image_bins(n)
    e = bins.shape[1]
    image = np.zeros((tables.shape[0], 64, e + 4), tables.dtype)
    image[:, :, :e] = tables[:, bins]
    flat, stride = image.reshape(-1), 64 * (e + 4)
    slot = c * stride - c + (np.arange(64)[:, None] * (e + 4) + np.arange(e))
    late = np.empty(tables.shape[-1], tables.dtype)
    late[bins] = flat[slot]
    return late


def strides(half):
    return [1 << s for s in range(half.bit_length() - 1)]


def pairs(n):
    """every (k, k + 2^s) inside the table with at least one probed member"""
    half = n // 2
    probed = np.zeros(half, bool)
    probed[probed_bins(n)] = True
    out = []
    for d in strides(half):
        k = np.arange(half - d)
        keep = probed[k] | probed[k + d]
        out.append(np.stack([k[keep], k[keep] + d], axis=1))
    return np.concatenate(out)


# ---- the power of the probe rows, in closed form ---------------------------------------------------------------------------
class Power:
    """Which single faults a set of rows shows.  m_ext[rows][N/2 + 1]: their fp64 magnitudes, the Nyquist bin last.  A fault
    is shown when it moves some row by POWER bounds under one of the targets; only the three rows in which a bin the
    fault touches is the loudest are asked (the Nyquist faults ask all), and only the slots it changes are evaluated."""

    def __init__(self, n, m_ext, targets, w, eps, r):
        self.n, self.half, self.eps = n, n // 2, eps
        self.m = np.asarray(m_ext, np.float64)
        self.t = np.concatenate([np.asarray(targets, np.float64), np.zeros((len(targets), 1))], axis=1)
        self.w = np.append(np.ones(self.half) if w is None else np.asarray(w, np.float64), 1.0)
        self.need = POWER * np.stack([bound(self.m[:, :-1], t[:-1], self.w[:-1], eps, r) for t in self.t])   # [targets][rows]
        self.rows = self.m.shape[0]
        self.near = np.argpartition(-self.m[:, :-1], min(2, self.rows - 1), axis=0)[:3].T

    def rows_near(self, k):
        """[len(k)][3] the rows in which bins k are the loudest"""
        return self.near[np.asarray(k)]

    def term(self, rows, mi, ti, wi, j):
        """w e^2 of slot (mi, ti, wi) in rows[.][c] under target j"""
        return self.w[wi][:, None] * errors(self.m[rows, np.asarray(mi)[:, None]], self.t[j][ti][:, None], self.eps) ** 2

    def shown(self, rows, change):
        """change(j) -> dF[faults][c] on rows[faults][c]; a fault is shown if any row under any target moves enough"""
        hit = np.zeros(rows.shape[0], bool)
        for j in range(len(self.t)):
            hit |= np.any(np.abs(change(j)) >= self.need[j][rows], axis=1)
        return hit

    def left_out(self, k):
        rows = self.rows_near(k)
        return self.shown(rows, lambda j: -self.term(rows, k, k, k, j))

    counted_twice = left_out                                 # +term: the same size

    def exchanged(self, pr, which):
        k, k2 = pr[:, 0], pr[:, 1]
        rows = np.concatenate([self.rows_near(k), self.rows_near(k2)], axis=1)
        if which == "targets":
            new = lambda j: self.term(rows, k, k2, k, j) + self.term(rows, k2, k, k2, j)
        else:
            new = lambda j: self.term(rows, k, k, k2, j) + self.term(rows, k2, k2, k, j)
        return self.shown(rows, lambda j: new(j) - self.term(rows, k, k, k, j) - self.term(rows, k2, k2, k2, j))

    def nyquist(self):
        """[added, in place of bin 0, in place of bin N/4]"""
        h = self.half
        every = np.arange(self.rows)[None, :]
        z, hh, q = np.array([0]), np.array([h]), np.array([h // 2])
        return np.concatenate([
            self.shown(every, lambda j: self.term(every, hh, hh, hh, j)),
            self.shown(every, lambda j: self.term(every, hh, z, z, j) - self.term(every, z, z, z, j)),
            self.shown(every, lambda j: self.term(every, hh, q, q, j) - self.term(every, q, q, q, j))])


def magnitudes_ext(O, audio):
    """fp64 normalised magnitudes [rows][N/2 + 1] of audio rows, the Nyquist bin last"""
    return np.concatenate([magnitudes(O, audio), nyquist_magnitude(O, audio)[:, None]], axis=1)


def tone_magnitudes(O, n):
    """m_ext of one pass through the tone set of N"""
    return magnitudes_ext(O, synthesise(O, probe_rows(n)[0], n))
