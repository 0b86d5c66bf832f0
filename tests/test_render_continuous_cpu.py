"""CPU checks of the phase-continuous rendering: the NumPy model against its own per-sample loop and
across pass sizes, one row against the CPU oracle's voice, the comb filter of the overlap-add rendering that it removes,
what the GPU tests' rows cover, the library's exports and the renderMode key of the host layer.  No GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _render_continuous_model as CM  # noqa: E402
import _render_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
HOST = os.path.join(PKG_DIR, "host")
PMAX, DIMS, track_rows = CM.PMAX, CM.DIMS, CM.track_rows


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def tab(O):
    return O.wavetable()


# ---- the model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("glide", [False, True])
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_loop_and_cumsum_forms_agree_bit_for_bit(tab, kind, glide):
    values = track_rows(kind, 6, 3 + kind)
    n, hop, samples = 64, 59, 300
    a = CM.render(kind, values, [0.0] * DIMS[kind], PMAX[kind], tab, n, hop, glide, out_samples=samples)
    b = CM.render_loop(kind, values, [0.0] * DIMS[kind], PMAX[kind], tab, n, hop, glide, out_samples=samples)
    assert np.array_equal(bits(a), bits(b))
    assert np.abs(a).max() > 0.01


@pytest.mark.parametrize("glide", [False, True])
def test_passes_give_the_same_bits(tab, glide):
    kind, n, hop = 1, 1024, 1000
    values = track_rows(kind, 7, 5)
    whole = CM.render(kind, values, [0.0] * 6, PMAX[kind], tab, n, hop, glide)
    assert len(whole) == 6 * hop + n
    for per_pass in (1, 1000, 4097):
        got = CM.render(kind, values, [0.0] * 6, PMAX[kind], tab, n, hop, glide, samples_per_pass=per_pass)
        assert np.array_equal(bits(got), bits(whole)), per_pass


def test_output_length(tab):
    values = track_rows(0, 3, 1)
    whole = CM.render(0, values, [0.0] * 4, PMAX[0], tab, 256, 100)
    assert len(whole) == 456
    longer = CM.render(0, values, [0.0] * 4, PMAX[0], tab, 256, 100, out_samples=470)
    assert np.array_equal(bits(longer[:456]), bits(whole)) and not bits(longer[456:]).any()
    assert np.array_equal(bits(CM.render(0, values, [0.0] * 4, PMAX[0], tab, 256, 100, out_samples=99)), bits(whole[:99]))


def test_hold_switches_half_way_and_glide_meets_the_rows(tab):
    values = np.array([[0.1] * 4, [0.5] * 4, [0.9] * 4], np.float32)
    n, hop = 64, 10
    idx = np.arange(CM.covered(3, n, hop))
    g = CM.genes(values, idx, n, hop, False)[:, 0]
    assert np.all(g[:32 + 5] == np.float32(0.1)) and np.all(g[32 + 5:32 + 15] == np.float32(0.5)) and np.all(g[32 + 15:] == np.float32(0.9))
    g = CM.genes(values, idx, n, hop, True)[:, 0]
    assert np.all(g[:33] == np.float32(0.1)) and g[42] == np.float32(0.5) and np.all(g[52:] == np.float32(0.9))
    assert np.all(np.diff(g[32:53]) > 0)


# One row: the output is that row's voice, but not the oracle's synth bit for bit - the phase has 17 fractional bits where
# fp32 has 8 near W.  It must stay close in the unit the matcher uses: the largest bin difference of the windowed magnitude
# spectra, relative to the largest bin.  Measured on these rows (32 rows, N = 2048, genes in [0.05, 0.95)): 0.00122 for the
# 2-op voice, 0.0148 for the 3-op voice; asserted: twice that, so that a change of definition shows and rounding noise does not.
@pytest.mark.parametrize("kind,seed,measured", [(0, 7, 0.00122), (1, 8, 0.0148)])
def test_one_row_is_the_oracles_voice_in_the_matchers_unit(O, tab, kind, seed, measured):
    n, d = 2048, DIMS[kind]
    worst = 0.0
    for v in M.unit_rows(32, d, seed):
        want = O.spectrum(O.synth(kind, v, [0.0] * d, PMAX[kind], n, tab))
        got = O.spectrum(CM.render(kind, v[None, :], [0.0] * d, PMAX[kind], tab, n, n))
        worst = max(worst, float(np.abs(got - want).max() / want.max()))
    print("kind %d: largest relative bin difference %.6f" % (kind, worst))
    assert worst <= 2.0 * measured


def test_a_stationary_tone_is_not_comb_filtered(O, tab):
    """40 identical pure-sine rows at 473.7 Hz, N = 2048, hop 512: successive rows are half a period apart, the overlap-add
    rendering cancels to silence, the continuous one is the sine (RMS 1 / sqrt 2)"""
    n, hop = 2048, 512
    row = np.array([[0.5, 0.0, 473.7 / 3520.0, 1.0]] * 40, np.float32)  # modulation index 0, amplitude 1
    ola = M.overlap_add(M.oracle_rows(O, 0, row, [0.0] * 4, PMAX[0], n), hop, M.window32(O, n))
    cont = CM.render(0, row, [0.0] * 4, PMAX[0], tab, n, hop)
    assert len(ola) == len(cont)
    assert CM.interior_rms(ola, n) < 0.01
    assert abs(CM.interior_rms(cont, n) - 2.0 ** -0.5) < 0.001
    glide = CM.render(0, row, [0.0] * 4, PMAX[0], tab, n, hop, glide=True)
    assert np.array_equal(bits(glide), bits(cont))  # identical rows: nothing to interpolate


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_the_gpu_tests_rows_cover_negative_and_wrapping_increments(tab, kind):
    wide = []
    CM.render(kind, track_rows(kind, 7, 100 * kind + 8), [0.0] * DIMS[kind], PMAX[kind], tab, 256, 64, wide=wide)
    lo, hi = min(int(w.min()) for w in wide), max(int(np.abs(w).max()) for w in wide)
    assert lo < 0, "no negative increment"
    assert hi >= 1 << 31, "no increment of magnitude 2^31 or more before the reduction"


def test_fix():
    x = np.array([0.0, 1.0, -1.0, 2.0 ** -18, 3 * 2.0 ** -18, 16384.0, -16384.0, 32768.0, 2.0 ** 44, 2.0 ** 45, -2.0 ** 45, np.inf, np.nan],
                 np.float32)
    want = [0, 1 << 17, (1 << 32) - (1 << 17), 0, 2, 1 << 31, 1 << 31, 0, 0, 0, 0, 0, 0]  # ties to even; |y| >= 2^62 and NaN: 0
    assert CM.fix(x).tolist() == want
    assert CM.fix_wide(np.float32(2.0 ** 44)) == 1 << 61


# ---- the library ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_point(hip):
    lib = hip.load()
    assert "sots_render_continuous" in hip.EXPORTS and hasattr(lib, "sots_render_continuous")
    assert ctypes.sizeof(hip.RenderContinuousArgs) == 16 and hip.RENDER_GLIDE == 1
    with open(os.path.join(ROOT, "include", "sots_hip.h")) as f:
        header = f.read()
    assert "int sots_render_continuous(" in header and "SOTS_RENDER_GLIDE = 1" in header


def test_argument_rules_are_clean_under_asan_and_ubsan(tmp_path):
    """render_continuous_check (csrc/sots_rules.h, pure host code) in a stand-alone program of its own"""
    exe = tmp_path / "render_continuous_rules_san"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unused-parameter", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-o", str(exe),
                           os.path.join(ROOT, "tests", "render_continuous_rules_san.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert out.stdout.strip() == "ok: 22 checks"


# ---- the host layer ----------------------------------------------------------------------------------------------------------
def test_render_mode_key(tmp_path):
    exe = tmp_path / "render_mode_test"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter",
                           "-o", str(exe), os.path.join(HOST, "render_mode_test.cpp")])
    good = {'{}': "given 0 renderMode 0", '{"renderMode": "overlapAdd"}': "given 1 renderMode 0",
            '{"renderMode": "continuous"}': "given 1 renderMode 1", '{"renderMode": "continuousGlide"}': "given 1 renderMode 2"}
    bad = ['{"renderMode": "Continuous"}', '{"renderMode": "glide"}', '{"renderMode": ""}', '{"renderMode": 1}', '{"renderMode": true}',
           '{"renderMode": null}', '{"renderMode": ["continuous"]}']
    out = subprocess.run([str(exe)] + list(good) + bad, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = dict(l[5:].split(" -> ", 1) for l in out.stdout.splitlines())
    assert len(got) == len(good) + len(bad)
    for text, want in good.items():
        assert got[text] == want, text
    for text in bad:
        assert got[text].startswith("refused: ") and "type.HIP.renderMode" in got[text], (text, got[text])
        assert '"overlapAdd", "continuous" or "continuousGlide"' in got[text]
    assert 'not "glide"' in got['{"renderMode": "glide"}']
