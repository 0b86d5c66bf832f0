"""CPU tests of the per-bin weights of the spectral objective (sots_set_objective_weights): the fp64 model the
GPU tests compare with, the header / library / binding's symbols, and the host's weight tables and its reading of
type.HIP.objectiveWeights (host/Objective_weights.hpp and host/Match_JSON.hpp, compiled with g++ here: no GPU and no
libsots_hip involved)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from _objective_model import log_distance, magnitudes
from _weights_model import fixed_weights, tolerance, weighted_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
HOST = os.path.join(PKG_DIR, "host")
PMAX = [3520.0, 8.0, 3520.0, 1.0]
NEW_SYMBOLS = ["sots_set_objective_weights", "sots_get_objective_weights", "sots_batch_set_objective_weights",
               "sots_group_set_objective_weights"]


@pytest.fixture(scope="module")
def rows(O):
    """64 random 2-op individuals of the oracle, N = 1024: audio and fp64 magnitudes"""
    v, _ = O.init_population(64, 4, 0x5EED0001)
    audio = np.stack([O.synth(0, v[i], [0.0] * 4, PMAX, 1024) for i in range(64)])
    return audio, magnitudes(O, audio)


def test_all_ones_is_the_oracles_fitness(rows, O):
    audio, m = rows
    ones = np.ones(512)
    t32 = O.spectrum(audio[63])
    for i in range(63):
        want = float(O.fitness(O.spectrum(audio[i]), t32))
        got = float(weighted_distance(m[i], m[63], ones))
        assert abs(got - want) <= 1e-5 * want, (i, got, want)


def test_all_ones_is_the_log_distance(rows):
    _, m = rows
    ones = np.ones(512)
    for eps in (1e-2, 1e-4):
        want = log_distance(m[:63], m[63], eps)
        got = weighted_distance(m[:63], m[63], ones, eps)
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)


def test_model_weights_scale_and_mask(rows):
    _, m = rows
    w = fixed_weights(1024)
    assert w.dtype == np.float32 and w.shape == (512,)
    assert np.all(w[128:257] == 0.0) and np.all(w[257:257 + 64] == 1.0) and w.min() >= 0.0 and w.max() <= 2.0
    for eps in (None, 1e-2):
        f = weighted_distance(m[:63], m[63], w, eps)
        np.testing.assert_allclose(weighted_distance(m[:63], m[63], 3.0 * w.astype(np.float64), eps), 3.0 * f, rtol=1e-13)
        other = m[63].copy()
        other[128:257] += 0.125                                     # the masked bins do not count
        assert np.array_equal(weighted_distance(m[:63], other, w, eps), f)
        assert np.all(tolerance(m[:63], m[63], w, eps, 2.5e-6) < 1e-2 * f)  # the GPU tests' bound is a fraction of F here


def test_exports_and_header_hold_the_new_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "sots_hip.h")).read()
    lib = pkg.capi.load()
    for name in NEW_SYMBOLS:
        assert name in pkg.capi.EXPORTS
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, header), name
    for cls in (pkg.HipES, pkg.HipBatch, pkg.HipGroup):
        assert callable(getattr(cls, "set_objective_weights"))
    assert callable(pkg.HipES.get_objective_weights)


DRIVER = r"""
#include <cstdio>
#include <fstream>
#include <sstream>
#include "Match_JSON.hpp"
// argv: N sampleRate file...   per file one line: "ok <given> <kind> <bins> <first one> <last one> <count of ones> <count of positives>"
int main(int argc, char **argv)
{
    const uint32_t N = (uint32_t)atoi(argv[1]);
    const double rate = atof(argv[2]);
    for (int i = 3; i < argc; ++i) {
        std::ifstream in(argv[i]);
        std::stringstream buf;
        buf << in.rdbuf();
        const std::string text = buf.str();
        try {
            const Json j = JsonParser(text).value();
            Objective_Weights_Spec spec;
            const bool given = readObjectiveWeightsKey(j["type"]["HIP"], spec);
            const std::vector<float> w = makeObjectiveWeights(spec, N, rate);
            int first = -1, last = -1, ones = 0, positive = 0;
            for (size_t k = 0; k < w.size(); ++k) {
                if (w[k] == 1.0f) { if (first < 0) first = (int)k; last = (int)k; ++ones; }
                if (w[k] > 0.0f) ++positive;
            }
            printf("ok %d %d %zu %d %d %d %d %s\n", (int)given, (int)spec.kind, w.size(), first, last, ones, positive, spec.describe().c_str());
        } catch (const std::exception &e) {
            printf("error %s\n", e.what());
        }
    }
    // the A-curve at the IEC table's frequencies, and through a table whose bins land on them: N = 4410 at 44100 Hz, bin k at 10 k Hz
    for (double f : {100.0, 1000.0, 2000.0, 10000.0, 20000.0}) printf("A %.0f %.6f\n", f, aWeightingDb(f));
    Objective_Weights_Spec a;
    a.kind = Objective_Weights_Spec::AWeighting;
    const std::vector<float> w = makeObjectiveWeights(a, 4410, 44100.0);
    for (int k : {0, 10, 100, 200, 1000, 2000}) printf("W %d %.9g\n", k, (double)w[k]);
    return 0;
}
"""


def test_host_weight_tables_and_json_key(tmp_path):
    src = tmp_path / "driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "driver"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", HOST, "-o", str(exe), str(src)])
    n, rate = 1024, 44100
    spacing = rate / n                                              # 43.07 Hz
    lo_bin, hi_bin = int(np.ceil(80 / spacing)), int(np.floor(6000 / spacing))
    band = hi_bin - lo_bin + 1
    table = [0.0] * 512
    table[7], table[9] = 0.5, 1.0
    nan_table, inf_table, neg_table = list(table), list(table), list(table)
    nan_table[3], inf_table[3], neg_table[3] = float("nan"), float("inf"), -0.25
    cases = [
        ({}, "ok 0 0 0 -1 -1 0 0 none"),                                           # no key: no table
        ({"objectiveWeights": {"bandHz": [80, 6000]}}, f"ok 1 1 512 {lo_bin} {hi_bin} {band} {band} bandHz 80 .. 6000"),
        ({"objectiveWeights": {"bandHz": [0, 43.0]}}, "ok 1 1 512 0 0 1 1 bandHz 0 .. 43"),        # bin 0 alone
        ({"objectiveWeights": {"bandHz": [spacing * 5, spacing * 6]}}, "ok 1 1 512 5 6 2 2 bandHz .*"),  # both ends inside
        ({"objectiveWeights": "aWeighting"}, r"ok 1 2 512 -1 -1 0 511 aWeighting"),   # w_0 = 0, every other bin positive
        ({"objectiveWeights": table}, "ok 1 3 512 9 9 1 2 table of 512 bins"),
        ({"objectiveWeights": {"bandHz": [6000, 80]}}, "error .*bandHz needs 0 <= lo < hi"),
        ({"objectiveWeights": {"bandHz": [500, 500]}}, "error .*bandHz needs 0 <= lo < hi"),
        ({"objectiveWeights": {"bandHz": [-5, 500]}}, "error .*bandHz needs 0 <= lo < hi"),
        ({"objectiveWeights": {"bandHz": [50, 80]}}, "error .*bandHz holds no bin"),               # between bins 1 and 2
        ({"objectiveWeights": {"bandHz": [30000, 40000]}}, "error .*bandHz holds no bin"),
        ({"objectiveWeights": {"bandHz": [80]}}, "error .*bandHz"),
        ({"objectiveWeights": {"band": [80, 6000]}}, "error .*bandHz"),
        ({"objectiveWeights": table[:511]}, "error .*needs 512 entries .*got 511"),
        ({"objectiveWeights": table + [1.0]}, "error .*needs 512 entries .*got 513"),
        ({"objectiveWeights": neg_table}, "error .*entry 3 must be finite and not negative"),
        ({"objectiveWeights": nan_table}, "error .*entry 3 must be finite and not negative"),     # (json writes NaN, strtod reads it)
        ({"objectiveWeights": inf_table}, "error .*entry 3 must be finite and not negative"),
        ({"objectiveWeights": [0.0] * 512}, "error .*at least one weight must be positive"),
        ({"objectiveWeights": "cWeighting"}, "error .*must be \"aWeighting\".*not \"cWeighting\""),
        ({"objectiveWeights": 3}, "error .*must be \"aWeighting\""),
    ]
    paths = []
    for i, (hip, _) in enumerate(cases):
        p = tmp_path / f"c{i}.json"
        p.write_text(json.dumps({"type": {"implementation": "HIP", "HIP": dict(hip, workgroupSize=32)}}))
        paths.append(str(p))
    # (JSON has no NaN or infinity: 1e999 reads as +infinity through strtod, and the table check sees it)
    p = tmp_path / "inf.json"
    p.write_text(json.dumps({"type": {"implementation": "HIP", "HIP": {"objectiveWeights": table}}}).replace("0.5", "1e999"))
    paths.append(str(p))
    cases.append(("1e999", "error .*entry 7 must be finite and not negative"))
    out = subprocess.run([str(exe), str(n), str(rate)] + paths, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(cases) + 11
    for (hip, want), got in zip(cases, lines):
        assert re.fullmatch(want if want.startswith("ok") else want + ".*", got), (hip, want, got)
    # the A-curve: the IEC table's values within 0.06 dB, and the formula's own to 1e-3
    iec = {100: (-19.1, -19.145), 1000: (0.0, 0.000), 2000: (1.2, 1.202), 10000: (-2.5, -2.492), 20000: (-9.3, -9.347)}
    got_a = {int(l.split()[1]): float(l.split()[2]) for l in lines if l.startswith("A ")}
    got_w = {int(l.split()[1]): float(l.split()[2]) for l in lines if l.startswith("W ")}
    assert sorted(got_a) == sorted(iec)
    for f, (table_db, formula_db) in iec.items():
        assert abs(got_a[f] - table_db) <= 0.06, (f, got_a[f])
        assert abs(got_a[f] - formula_db) <= 1e-3, (f, got_a[f])
        db = 10.0 * np.log10(got_w[f // 10])                         # the table's bin at f: w = 10^(A / 10)
        assert abs(db - table_db) <= 0.06, (f, db)
    assert got_w[0] == 0.0


def test_library_checks_match_the_host_checks():
    """the C-ABI's validity rules are stated once for contexts and batches (objective_weights_check) and refuse what the
    host's table maker refuses: negative, non-finite, all zero, wrong length.  Once: one definition in one header of
    csrc/, and one call in all of csrc/*.h and csrc/*.hip, which contexts and batches both reach."""
    import glob
    import re
    csrc = os.path.join(PKG_DIR, "csrc")
    defined, called = [], []
    for path in sorted(glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.hip"))):
        code = re.sub(r"//[^\n]*", "", open(path).read())       # (comments may name it)
        n_def = code.count("inline int objective_weights_check(")
        defined += [os.path.basename(path)] * n_def
        called += [os.path.basename(path)] * (code.count("objective_weights_check(") - n_def)
    assert len(defined) == 1 and defined[0].endswith(".h"), defined
    assert len(called) == 1, called


def test_sots_match_source_prints_the_weights_only_when_asked():
    """without the key the driver's output is what it was: the one extra line sits behind objectiveWeights.given()"""
    text = open(os.path.join(HOST, "sots_match.cpp")).read()
    assert text.count('printf("Objective weights: ') == 1
    i = text.index('printf("Objective weights: ')
    assert "if (args.objectiveWeights.given())" in text[i - 200:i]
