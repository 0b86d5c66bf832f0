"""CPU checks of the overlap-add rendering: the NumPy model's own properties on the CPU oracle's rows,
the library's exports, the hopSize key and the chunk count formula of the host layer, and the parameter track's number
format.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
HOST = os.path.join(PKG_DIR, "host")
PMAX = [3520.0, 8.0, 3520.0, 1.0]
N, ROWS = 1024, 7
NEW_SYMBOLS = ["sots_render_overlap_add", "sots_batch_set_target_audio_hop", "sots_batch_queue_targets_audio_hop"]


@pytest.fixture(scope="module")
def rows(O):
    return M.oracle_rows(O, 0, M.unit_rows(ROWS, 4, 1), [0.0] * 4, PMAX, N)


# ---- the model ---------------------------------------------------------------------------------------------------------
def test_rectangular_at_hop_n_is_the_rows_end_to_end(rows):
    out = M.overlap_add(rows, N)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), rows.reshape(-1).view(np.uint32))


def test_window_table(O):
    w = M.window32(O, N)
    assert w.dtype == np.float32 and w[0] == 0.0 and w.max() == 2.0 and w[N // 2] == 2.0
    assert np.all(w[1:] > 0.0)
    assert np.allclose(w[1:], w[:0:-1], rtol=1e-6, atol=0)  # periodic: w[n] = w[N - n]


@pytest.mark.parametrize("hop", [1024, 512, 384, 256, 100, 16])
def test_windowed_denominator_and_bounds(O, rows, hop):
    w = M.window32(O, N)
    acc, den = M.accumulate(rows, hop, w)
    assert len(den) == (ROWS - 1) * hop + N
    zero = np.flatnonzero(den == 0)
    # w[0] = 0: a sample is left without weight only where the one chunk covering it starts
    want = np.arange(ROWS) * N if hop == N else np.array([0])
    assert np.array_equal(zero, want)
    assert den[den > 0].min() >= np.float32(1.8e-5)  # 1 - cos(2 pi / 1024) = 1.88e-5
    out = M.overlap_add(rows, hop, w)
    assert np.all(np.isfinite(out)) and np.all(out[zero] == 0)
    assert np.abs(out).max() <= np.abs(rows).max()  # a weighted mean of the rows' samples
    longer = M.overlap_add(rows, hop, w, out_samples=len(out) + 9)
    assert np.array_equal(longer[:len(out)], out) and not longer[len(out):].view(np.uint32).any()
    assert np.array_equal(M.overlap_add(rows, hop, w, out_samples=len(out) - 9), out[:-9])


def test_model_order_is_ascending_chunks(O, rows):
    """a per-sample restatement with an explicit ascending loop gives the model's bits"""
    hop, w = 100, M.window32(O, N)
    out = M.overlap_add(rows, hop, w)
    for n in (0, 1, 99, 100, 555, 1023, 1024, 1300, len(out) - 1):
        acc = den = np.float32(0)
        for c in range(ROWS):
            if c * hop <= n < c * hop + N:
                acc = np.float32(acc + np.float32(w[n - c * hop] * rows[c][n - c * hop]))
                den = np.float32(den + w[n - c * hop])
        want = np.float32(acc / den) if den > 0 else np.float32(0)
        assert out[n].view(np.uint32) == want.view(np.uint32), n


def test_wav_quantisation_restated():
    x = np.array([0.5, 1.0, -1.0, 1e-8, -1e-8, 0.3, -0.3, 2.0, -2.0], np.float32)
    q = M.quantise_24bit(x) * 8388608.0
    assert np.array_equal(q, [4194304, 8388607, -8388608, 0, 0, 2516582, -2516582, 8388607, -8388608])


# ---- the library ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points(hip):
    lib = hip.load()
    for name in NEW_SYMBOLS:
        assert name in hip.EXPORTS
        assert hasattr(lib, name), name
    assert ctypes.sizeof(hip.RenderArgs) == 16 and hip.RENDER_WINDOWED == 1
    with open(os.path.join(ROOT, "include", "sots_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header


# ---- the host layer ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("matchtrack")
    exe = d / "match_track_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-o", str(exe), os.path.join(HOST, "match_track_test.cpp")])
    rng = np.random.default_rng(5)
    bits = np.concatenate([np.array([0x00000000, 0x3F800000, 0x3F7FFFFF, 0x3DCCCCCD, 0x00800000, 0x00000001, 0x3EAAAAAB, 0x33800000],
                                    np.uint32), rng.uniform(0, 1, 56).astype(np.float32).view(np.uint32)])
    csv = d / "track.csv"
    out = subprocess.run([str(exe), str(csv)] + ["%08x" % b for b in bits], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines(), csv, bits


def test_hop_size_key(host):
    lines, _, _ = host
    got = {l.split(" -> ")[0][4:]: l.split(" -> ")[1] for l in lines if l.startswith("hop {")}
    assert got["{}"] == "given 0 hopSize 0 hop 1024"
    assert got['{"hopSize": 0}'] == "given 1 hopSize 0 hop 1024"
    assert got['{"hopSize": 1024}'] == "given 1 hopSize 1024 hop 1024"
    assert got['{"hopSize": 512}'] == "given 1 hopSize 512 hop 512"
    assert got['{"hopSize": 101}'] == "given 1 hopSize 101 hop 101"
    assert got['{"hopSize": 16}'] == "given 1 hopSize 16 hop 16"
    for bad in ("15", "1025", "-512", "100.5", '"512"', "1e99", "true"):
        text = got['{"hopSize": %s}' % bad]
        assert text.startswith("refused: ") and "type.HIP.hopSize" in text, (bad, text)
    assert "16 .. 1024" in got['{"hopSize": 15}']
    low = [l for l in lines if l.startswith("hop200 ")]
    assert low == ["hop200 3 -> refused", "hop200 4 -> 4", "hop200 5 -> 5"]  # ceil(200 / 64) = 4


def test_chunk_count_formula(host):
    lines, _, _ = host
    seen = 0
    for l in lines:
        if not l.startswith("chunks "):
            continue
        L, n, hop, count, covered = (int(x) for x in l.split()[1:])
        want = 0 if L < n else (L - n) // hop + 1
        assert count == want, l
        assert covered == (0 if want == 0 else (want - 1) * hop + n), l
        assert covered <= L
        if hop == n:
            assert count == L // n  # the reference's chunking
        seen += 1
    assert seen == 40


def test_track_numbers_give_the_bits_back(host):
    _, csv, bits = host
    with open(csv) as f:
        text = f.read().splitlines()
    assert text[0] == "chunk,start_sample,generations,fitness,u0,u1,u2,u3,p0,p1,p2,p3"
    assert len(text) == 1 + len(bits) // 4
    for r, line in enumerate(text[1:]):
        cells = line.split(",")
        assert len(cells) == 12
        assert (int(cells[0]), int(cells[1]), int(cells[2])) == (r, 512 * r, 20 + r)
        u = np.array([float(c) for c in cells[4:8]]).astype(np.float32)
        assert np.array_equal(u.view(np.uint32), bits[4 * r:4 * r + 4]), line
        assert np.float32(float(cells[3])).view(np.uint32) == bits[4 * r]
        p = np.array([float(c) for c in cells[8:12]]).astype(np.float32)
        assert np.array_equal(p, bits[4 * r:4 * r + 4].view(np.float32) * np.float32(3520.0))


# ---- the pass and index arithmetic of the device path, restated --------------------------------------------------------------
def render_as_the_device_does(rows_audio, hop, w, rows_per_pass, out_samples):
    """sots_render_overlap_add's pass loop (csrc/sots_capi.hip) and k_overlap_add's index arithmetic (csrc/sots_render.hip) line by
    line: scratch rows pitch apart and NaN wherever nothing was synthesised, every load asserted to stay inside its row"""
    num_rows, n = rows_audio.shape
    pitch = n + 32
    reach = (n + hop - 1) // hop - 1
    step = min(rows_per_pass if rows_per_pass else 4096, num_rows)
    covered = (num_rows - 1) * hop + n
    want = min(out_samples, covered)
    out = np.full(out_samples, np.nan, np.float32)
    r0 = 0
    while r0 < num_rows and r0 * hop < want:
        r1 = r0 + step if num_rows - r0 > step else num_rows
        first = r0 - reach if r0 > reach else 0
        rows = r1 - first
        assert rows <= step + reach
        s0 = r0 * hop
        end = min(want if r1 == num_rows else r1 * hop, want)
        count = end - s0
        assert count > 0
        audio = np.full(rows * pitch, np.nan, np.float32)
        for l in range(rows):
            audio[l * pitch:l * pitch + n] = rows_audio[first + l]
        out_first, quads, vec = (r0 - first) * hop, (count + 3) // 4, hop % 4 == 0
        assert 4 * quads <= step * hop + n + 4 and (not vec or out_first % 4 == 0)
        o = np.zeros(4 * quads, np.float32)
        for q in range(quads):
            s = out_first + 4 * q
            for k in range(4):
                sk = s + k
                base = s if vec else sk  # the vector path takes the quad's chunks from its first sample
                lo = (base - n) // hop + 1 if base >= n else 0
                hi = min(base // hop, rows - 1)
                acc = den = np.float32(0)
                for l in range(lo, hi + 1):
                    off = sk - l * hop
                    assert 0 <= off < n
                    a = audio[l * pitch + off]
                    assert not np.isnan(a)
                    ww = np.float32(1) if w is None else w[off]
                    acc, den = np.float32(acc + np.float32(ww * a)), np.float32(den + ww)
                o[4 * q + k] = np.float32(acc / den) if den > 0 else 0
        out[s0:s0 + count] = o[:count]
        r0 += step
    out[covered:] = 0
    return out


@pytest.mark.parametrize("num_rows", [1, 7])
def test_pass_and_index_arithmetic_give_the_model(num_rows):
    n = 64
    rng = np.random.default_rng(num_rows)
    audio = rng.standard_normal((num_rows, n)).astype(np.float32)
    w = (1 - np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)
    w[0] = 0
    for hop in (64, 32, 16, 5, 1, 63):
        covered = (num_rows - 1) * hop + n
        for window in (w, None):
            for per_pass in (0, 1, 3):
                for length in (covered, covered - 5, covered + 5):
                    got = render_as_the_device_does(audio, hop, window, per_pass, length)
                    want = M.overlap_add(audio, hop, window, out_samples=length)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (hop, window is None, per_pass, length)
