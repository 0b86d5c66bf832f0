"""CPU tests of the selectable spectral objective (sots_set_objective): the fp64 model the GPU tests compare with, the
binding's export list, and the host's reading of type.HIP.objective / type.HIP.objectiveFloor (host/Match_JSON.hpp, compiled
with g++ here: no GPU and no libsots_hip involved)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from _objective_model import log_distance, magnitudes, tolerance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
HOST = os.path.join(PKG_DIR, "host")
PMAX = [3520.0, 8.0, 3520.0, 1.0]
NEW_SYMBOLS = ["sots_set_objective", "sots_get_objective", "sots_batch_set_objective", "sots_group_set_objective"]


@pytest.fixture(scope="module")
def rows(O):
    """64 random 2-op individuals of the oracle, N = 1024: audio and fp64 magnitudes"""
    v, _ = O.init_population(64, 4, 0x5EED0001)
    audio = np.stack([O.synth(0, v[i], [0.0] * 4, PMAX, 1024) for i in range(64)])
    return audio, magnitudes(O, audio)


def test_model_self_distance_is_zero(rows):
    _, m = rows
    for eps in (1e-2, 1e-4, 1e-30, 1.0):
        assert np.all(log_distance(m, m[0], eps)[0] == 0.0)
        assert log_distance(m[5], m[5], eps) == 0.0
    assert np.all(log_distance(m[1:], m[0], 1e-3) > 0.0)


def test_model_linear_limit_is_the_oracles_fitness(rows, O):
    """eps -> infinity: ln(m + eps) - ln(t + eps) -> (m - t) / eps, so eps^2 F_log is the linear sum of squares"""
    audio, m = rows
    eps = 1e6
    t32 = O.spectrum(audio[63])
    for i in range(63):
        want = float(O.fitness(O.spectrum(audio[i]), t32))
        got = float(log_distance(m[i], m[63], eps)) * eps * eps
        assert abs(got - want) <= 1e-5 * want, (i, got, want)


def test_model_magnitudes_are_the_oracles_spectrum(rows, O):
    audio, m = rows
    for i in (0, 17, 63):
        np.testing.assert_allclose(m[i], O.spectrum(audio[i]), rtol=0, atol=np.spacing(np.float32(0.5)))


def test_tolerance_is_small_where_the_tests_use_it(rows):
    """the bound of the GPU tests, on the oracle's rows against the 64th: a fraction of F at the floors they use"""
    _, m = rows
    for eps, cap in ((1e-2, 1e-2), (1e-4, 1e-2)):
        f = log_distance(m[:63], m[63], eps)
        tol = tolerance(m[:63], m[63], eps, 2.5e-6)  # the GPU tests' LAMBDA
        assert np.all(tol < cap * f), (eps, float(np.max(tol / f)))


def test_exports_and_header_hold_the_new_symbols(pkg):
    header = open(os.path.join(ROOT, "include", "sots_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in pkg.capi.EXPORTS
        assert re.search(r"\bint %s\(" % name, header), name
    assert (pkg.capi.OBJECTIVE_MAGNITUDE, pkg.capi.OBJECTIVE_LOG_MAGNITUDE) == (0, 1)
    assert re.search(r"SOTS_OBJECTIVE_MAGNITUDE = 0, SOTS_OBJECTIVE_LOG_MAGNITUDE = 1", header)
    for cls in (pkg.HipES, pkg.HipBatch, pkg.HipGroup):
        assert callable(getattr(cls, "set_objective"))
    assert isinstance(pkg.HipES.objective, property)


DRIVER = r"""
#include <cstdio>
#include <fstream>
#include <sstream>
#include "Match_JSON.hpp"
int main(int argc, char **argv)
{
    for (int i = 1; i < argc; ++i) {
        std::ifstream in(argv[i]);
        std::stringstream buf;
        buf << in.rdbuf();
        const std::string text = buf.str();
        try {
            const Json j = JsonParser(text).value();
            uint32_t objective = 7;
            float floor = -1.0f;
            const bool given = readObjectiveKeys(j["type"]["HIP"], objective, floor);
            printf("ok %d %u %.9g\n", (int)given, objective, (double)floor);
        } catch (const std::exception &e) {
            printf("error %s\n", e.what());
        }
    }
    return 0;
}
"""


def test_json_keys_are_read_and_checked(tmp_path):
    src = tmp_path / "driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "driver"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", HOST, "-o", str(exe), str(src)])
    cases = [
        ({}, "ok 0 7 -1"),                                                        # no keys: nothing is touched
        ({"objective": "magnitude"}, "ok 1 0 0"),
        ({"objective": "magnitude", "objectiveFloor": 0.5}, "ok 1 0 0"),          # the floor is ignored and reported as 0
        ({"objective": "logMagnitude", "objectiveFloor": 1e-3}, "ok 1 1 0.00100000005"),
        ({"objective": "logMagnitude", "objectiveFloor": 1.0}, "ok 1 1 1"),
        ({"objective": "logMagnitude", "objectiveFloor": 1e-30}, "ok 1 1 1e-30"),
        ({"objectiveFloor": 1e-3}, "ok 1 0 0"),
        ({"objective": "logMagnitude"}, "error .*needs type.HIP.objectiveFloor"),
        ({"objective": "power", "objectiveFloor": 1e-3}, "error .*objective must be .*not \"power\""),
        ({"objective": 1, "objectiveFloor": 1e-3}, "error .*objective must be"),
        ({"objective": "logMagnitude", "objectiveFloor": 0.0}, "error .*objectiveFloor must lie in 1e-30 .. 1"),
        ({"objective": "logMagnitude", "objectiveFloor": -1e-3}, "error .*objectiveFloor must lie"),
        ({"objective": "logMagnitude", "objectiveFloor": 1.5}, "error .*objectiveFloor must lie"),
        ({"objective": "logMagnitude", "objectiveFloor": 1e-31}, "error .*objectiveFloor must lie"),
        ({"objective": "logMagnitude", "objectiveFloor": "small"}, "error .*number expected"),
    ]
    paths = []
    for i, (hip, _) in enumerate(cases):
        p = tmp_path / f"c{i}.json"
        p.write_text(json.dumps({"type": {"implementation": "HIP", "HIP": dict(hip, workgroupSize=32)}}))
        paths.append(str(p))
    out = subprocess.run([str(exe)] + paths, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(cases)
    for (hip, want), got in zip(cases, lines):
        assert re.fullmatch(want if want.startswith("ok") else want + ".*", got), (hip, want, got)


def test_sots_match_source_prints_the_objective_only_when_asked():
    """without the keys the driver's output is what it was: the one extra line sits behind objectiveGiven"""
    text = open(os.path.join(HOST, "sots_match.cpp")).read()
    assert text.count('printf("Objective: ') == 1
    i = text.index('printf("Objective: ')
    assert "if (args.objectiveGiven)" in text[i - 200:i]
