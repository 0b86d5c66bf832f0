"""NumPy model of the LIST MODE of the one-launch selection: the kernel that computes the fitness files every
key under its bucket between the stored splitters - per-bucket lists of CAP places and counters - and a selection
workgroup reads its bucket from there instead of streaming all P keys.  No GPU: this pins what the kernels are written to.
The bucket of a key is the number of sanitised bounds t_q (q >= 1) with t_q <= key, normalised or not; keys arrive in ANY
order; a bucket's CAP places are SHARDS segments with a counter each, and a key goes to the segment of the workgroup that
files it (one counter word takes only so many atomics per microsecond); a counter counts every key of its segment, also
beyond its CAP / SHARDS places, where only the store is skipped; the open last bucket is never filed (it is P minus the
closed ones); a workgroup with an overflowed segment, or that owns the open bucket, streams as without lists.  The
positions are the stable sort's whatever the slot holds."""
import numpy as np
import pytest

from test_gpu_parity import fitness_pattern
from test_select_splitters_model import (PATTERNS, SPLITTER_KINDS, make_keys, model_select, normalise, rank_step, sanitise,
                                         splitters)

STALE = np.uint64(0xDEADBEEFDEADBEEF)  # what an older generation left in a list: never looked at
SHARDS = 16


def shard_of(rows):
    """the segment a row's key is filed in: its filing workgroup's number mod SHARDS (here: runs of four rows in turn)"""
    return (np.asarray(rows) // 4) % SHARDS


def bucket_of(keys, slot):
    """the number of bounds t_q, q >= 1, with t_q <= key (bkt_visit): by the normalised bounds, as the kernels compare"""
    t = sanitise(slot)
    tn = np.array([normalise(x) for x in t], np.uint64)
    j = np.searchsorted(tn[1:], keys, side="right")
    assert np.array_equal(j, np.searchsorted(t[1:], keys, side="right")), "normalising a bound moved a key across it"
    assert np.all(np.diff(tn.astype(object)) >= 0)
    return j


def file_keys(f, slot, cap, rng):
    """the filing kernel: keys in a shuffled order (whichever wavefront finishes first), counters past CAP, nothing for
    the open bucket"""
    keys = make_keys(f)
    B = len(slot)
    j = bucket_of(keys, slot)
    seg = cap // SHARDS
    cnt = np.zeros((B, SHARDS), np.int64)  # the invariant: all zero when the filing launch starts
    lists = np.full((B, SHARDS, seg), STALE, np.uint64)
    sh = shard_of(np.arange(len(f)))
    for i in rng.permutation(len(f)):
        b = j[i]
        if b >= B - 1:
            continue
        pos = cnt[b, sh[i]]
        cnt[b, sh[i]] += 1
        if pos < seg:
            lists[b, sh[i], pos] = keys[i]
    assert np.all(cnt[B - 1] == 0) and np.all(lists[B - 1] == STALE), "the open bucket is never filed"
    return cnt, lists


def model_select_lists(f, slot, step, need, cap, rng):
    """k_sel_splitters with lists, workgroup by workgroup: position and size from the counters, the bucket from the list
    (fast path) or from a stream of all keys (list overflowed / the open bucket).  Every bucket is ordered here, also
    those the kernel leaves alone, to check every position."""
    keys = make_keys(f)
    B, P = len(slot), len(f)
    shards, lists = file_keys(f, slot, cap, rng)
    cnt = shards.sum(axis=1)
    t = sanitise(slot)
    perm = np.full(P, -1, np.int64)
    nxt = np.zeros(B, np.uint64)
    paths = []
    for j in range(B):
        last = j + 1 == B
        c = int(cnt[:j].sum())
        n = P - c if last else int(cnt[j])
        if last or np.any(shards[j] > cap // SHARDS):  # the stream, by the bounds made from the slot
            inside = keys >= t[j]
            if not last:
                inside &= keys < t[j + 1]
            assert int(np.sum(keys < t[j])) == c and int(inside.sum()) == n, "the counters say what the stream says"
            bucket = np.sort(keys[inside])
            paths.append("stream")
        else:
            bucket = np.sort(np.concatenate([lists[j, g, :shards[j, g]] for g in range(SHARDS)]))  # the segments one behind the other
            assert len(bucket) == n
            assert not np.any(bucket == STALE)
            paths.append("list")
        pos = c + np.arange(n)
        assert np.all(perm[pos] == -1)
        perm[pos] = (bucket & np.uint64(0xFFFFFFFF)).astype(np.int64)
        q = pos // step
        take = (pos % step == 0) & (q >= 1) & (q < B)
        if last and c >= need:
            nxt[-(-c // step):] = t[j]
        else:
            nxt[q[take]] = bucket[take]
    return perm, nxt, cnt, paths


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", SPLITTER_KINDS)
def test_list_mode_positions_are_exact_for_any_splitters(O, pattern, kind):
    P, B, need, cap = 4096, 64, 1024, 128
    step = rank_step(need, B)
    rng = np.random.default_rng(len(pattern) * 31 + len(kind))
    f = fitness_pattern(pattern, P, rng)
    slot = splitters(kind, B, P, step, f, rng)
    perm, nxt, cnt, paths = model_select_lists(f, slot, step, need, cap, rng)
    assert np.array_equal(perm, O.sort_perm(f))
    perm0, nxt0, sizes0 = model_select(f, slot, step, need)  # the streaming model: same buckets, same next slot
    assert np.array_equal(nxt, nxt0) and list(cnt[:-1]) == sizes0[:-1] and P - cnt.sum() == sizes0[-1]
    if kind == "fresh":
        assert paths[:-1].count("list") == B - 1, "good splitters: every closed bucket is served by its list"
    if kind == "ones":
        assert cnt[0] == P and paths[0] == "stream", "everything in bucket 0: its list overflows"
    if kind == "zero":
        assert cnt.sum() == 0, "everything in the open bucket: nothing is filed"


@pytest.mark.parametrize("extra", [0, 1])
def test_a_bucket_of_exactly_cap_keys_and_one_more(O, extra):
    """CAP keys that fill every segment to its last place are served from the list; with one key more a segment counts
    one more than it stores, and the workgroup streams.  (Rows in index order: consecutive rows take the shards in turn.)"""
    P, B, need, cap = 4096, 64, 1024, 128
    step = rank_step(need, B)
    rng = np.random.default_rng(17 + extra)
    f = fitness_pattern("ascending", P, rng)
    k = np.sort(make_keys(f))
    w = 32  # (bucket 5 then starts at row 160, where a run of four rows starts)
    slot = k[np.arange(B) * w].copy()       # buckets of w keys ...
    slot[6:] = k[5 * w + cap + extra + (np.arange(6, B) - 6) * w]  # ... but bucket 5: exactly cap (+ extra) keys
    perm, nxt, cnt, paths = model_select_lists(f, slot, step, need, cap, rng)
    assert cnt[5] == cap + extra and paths[5] == ("stream" if extra else "list")
    assert np.array_equal(perm, O.sort_perm(f))
    assert np.array_equal(nxt, model_select(f, slot, step, need)[1])

