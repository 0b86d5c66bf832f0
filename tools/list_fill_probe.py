"""Diagnostic: how full the key lists of the selection's list mode get in a real run.  A bucket's list is
16 segments of 128 places, a row's key goes to segment (row mod grid) mod 16 = row mod 16 (the wide spectral kernel deals
row b + t grid to workgroup b, the grid is a multiple of 16), and a workgroup of the selection falls back to streaming
when one of its segments overflows.  The library does not report that, but the host can count it exactly: before every
generation it reads the slot the selection will use, after it the unsorted half's fitness, and files the keys itself.
usage: python tools/list_fill_probe.py [generations]   (configs[2]: 16384 + 49152, 2-op, N = 1024)"""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")
import bench
from test_select_splitters_model import make_keys, normalise, sanitise

gens = int(sys.argv[1]) if len(sys.argv) > 1 else 220
SHARDS, SEG = 16, 128
# the context and target of a plain `python bench.py`
es = pkg.HipES(16384, 49152, pkg.capi.SYNTH_NAMES["2op"], 10, None, bench.VOICES["2op"][0], seed=0x5EED0001, workgroup_size=32)
es.set_target_audio(bench.make_target(pkg, "2op", 10, 0))
es.init_population(0)
es.execute_generations(1)  # the first generation runs TILES and seeds the slot
B = es.select_splitter_count()
worst, overflowing, closed_keys, open_rows = [], [], [], []
for g in range(gens):
    slot = es.read_select_splitters()
    es.execute_generations(1)
    f = es.read_population(other=True)[2]  # the half the selection read
    keys = make_keys(f)
    tn = np.array([normalise(x) for x in sanitise(slot)], np.uint64)
    j = np.searchsorted(tn[1:], keys, side="right")
    closed = j < B - 1
    fill = np.zeros((B, SHARDS), np.int64)
    np.add.at(fill, (j[closed], np.arange(len(f))[closed] % SHARDS), 1)
    worst.append(int(fill.max())); overflowing.append(int((fill.max(axis=1) > SEG).sum()))
    closed_keys.append(int(closed.sum())); open_rows.append(int((np.sort(keys)[:16384] >= tn[-1]).sum()))
    if g < 8 or g % 20 == 0 or overflowing[-1] or open_rows[-1]:
        print(f"generation {g + 2:4d}: closed keys {closed_keys[-1]:6d}  fullest segment {worst[-1]:4d} of {SEG}  buckets with an overflowed "
              f"segment {overflowing[-1]}  selected rows in the open bucket {open_rows[-1]}")
print(f"{gens} generations: fullest segment {max(worst)} of {SEG}; generations with an overflowed segment {sum(1 for x in overflowing if x)}; "
      f"generations whose open bucket held selected rows (its workgroup streams) {sum(1 for x in open_rows if x)}")
es.close()
