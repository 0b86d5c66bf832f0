"""The two-level bucket lookup of the key-filing kernels without a GPU: the bound-table index map (q mod 4) * 64 + q div 4
and the count -> bucket formula are one host-callable statement (csrc/sots_bkt_layout.h) that the kernels and
tests/filing_model_host.cpp share; the program takes a wavefront's steps through it (open bucket first, 64 group ends,
the four bounds of one group) and must name, for every key, the bucket brute force names: the number of bounds at or
below the key, minus one."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "filing_model_host.cpp")
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
SIZES = [2, 3, 4, 5, 64, 255, 256]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("filing") / "filing_model_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", str(out), SRC])
    return str(out)


def run(exe, bounds, keys):
    text = "%x\n" % len(bounds) + " ".join("%x" % int(t) for t in bounds) + "\n%x\n" % len(keys) + "\n".join("%x" % int(k) for k in keys) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.split("\n")
    return np.array(lines[0].split(), np.int64), np.array(lines[1:1 + len(keys)], np.int64)


def brute(bounds, keys):
    """the number of bounds at or below the key, minus one (t_0 = 0 is at or below every key)"""
    t = np.array(bounds, np.uint64)
    t[0] = 0
    return np.array([int(np.sum(t <= k)) - 1 for k in keys], np.int64)


def bound_sets(B, rng):
    yield "random", np.sort(rng.integers(0, 1 << 63, B, dtype=np.uint64) * np.uint64(2))
    yield "equal", np.full(B, 0x3F80000000000123, np.uint64)
    yield "zero", np.zeros(B, np.uint64)
    yield "ones", np.full(B, ONES, np.uint64)
    yield "dense", np.uint64(0x4000000000000000) + np.arange(B, dtype=np.uint64)  # neighbours: the row index word decides
    pairs = np.sort(rng.integers(0, 1 << 63, (B + 1) // 2, dtype=np.uint64))
    yield "pairs", np.repeat(pairs, 2)[:B]                                          # every bound twice
    low = np.sort(rng.integers(0, 1 << 31, B, dtype=np.uint64)) | np.uint64(0x80000000)
    yield "bit31", (np.uint64(0xBF000000) << np.uint64(32)) | low                   # low words with the top bit set


def keys_for(bounds, rng):
    """every bound, its neighbours on both sides, the ends of the key range and random keys (a key is never all-ones)"""
    t = np.array(bounds, np.uint64)
    k = np.concatenate([t, t - np.uint64(1), t + np.uint64(1), np.array([0, 1, int(ONES) - 1], np.uint64),
                        rng.integers(0, 1 << 63, 64, dtype=np.uint64) * np.uint64(2) + np.uint64(1)])
    return k[k != ONES]


def test_index_map_is_the_stated_one_and_a_permutation(exe):
    slots, _ = run(exe, np.zeros(2, np.uint64), np.zeros(1, np.uint64))
    q = np.arange(256)
    assert np.array_equal(slots, (q % 4) * 64 + q // 4)
    assert np.array_equal(np.sort(slots), q)
    # member c of every group side by side; the last bound of group l at 192 + l
    assert np.array_equal(slots[3::4], 192 + np.arange(64))


@pytest.mark.parametrize("B", SIZES)
def test_two_level_lookup_equals_brute_force(exe, B):
    rng = np.random.default_rng(30 + B)
    for name, bounds in bound_sets(B, rng):
        assert np.all(np.diff(bounds.astype(object)) >= 0), name
        keys = keys_for(bounds, rng)
        _, got = run(exe, bounds, keys)
        want = brute(bounds, keys)
        assert np.array_equal(got, want), f"B = {B}, {name}: first difference at key {keys[np.argmax(got != want)]:#x}"
        assert got.min() >= 0 and got.max() <= B - 1
