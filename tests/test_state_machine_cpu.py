"""The sequence tests' generator, legality rules and normaliser (tests/_state_machine.py), without a GPU: every list is
run on a context that computes nothing, keeps the state sots_capi.hip keeps, and raises on a call whose result the header
leaves unspecified - and the committed seeds are held to the situations they must contain."""
import numpy as np
import pytest

import _state_machine as SM

SHAPES = list(SM.SHAPES)
SWEEP = 2000


def drive(shape, ops, role):
    sh = SM.Shape(shape)
    f = SM.FakeContext(sh, role)
    for op in ops:
        SM.apply(f, op, sh)
    return f


@pytest.mark.parametrize("shape", SHAPES)
def test_the_same_seed_gives_the_same_list(shape):
    for seed in SM.SEEDS[shape][:3]:
        a, sa, ba = SM.generate(shape, seed)
        b, sb, bb = SM.generate(shape, seed)
        assert a == b and sa == sb and ba == bb
        assert SM.generate(shape, seed + 1)[0] != a
    assert len(set(SM.SEEDS[shape])) == 12


@pytest.mark.parametrize("shape", SHAPES)
def test_no_illegal_operation_is_emitted_and_b_sees_only_its_own(shape):
    """2000 seeds: the fake context raises Illegal on a stage that reads rows SORT_TOP_ONLY left unspecified, a partial
    write into them, a stage whose input does not exist, a call that needs a target before there is one, a call between
    select and rotate, a setting the voice does not take - and, as B, on every call B must not see.  Every refusal must be
    refused with its code."""
    sh = SM.Shape(shape)
    for seed in range(SWEEP):
        ops, _, _ = SM.generate(shape, seed)
        assert len(ops) in (SM.OPS, SM.OPS + 1) and ops[SM.OPS - 1][0] == "checkpoint"
        assert ops[-1][0] in ("checkpoint", "final_lazy")
        a = drive(shape, ops, "A")
        if ops[-1][0] == "final_lazy":  # only where the rest can still be produced
            assert a.tail_defined and ops[-2][1] == sh.S
        else:
            assert ops[-1][1] == sh.P
        b_ops = SM.normalise(ops)
        assert not [op for op in b_ops if op[0] in SM.NOT_FOR_B]
        b = drive(shape, b_ops, "B")
        assert b.mode == SM.SORT_FULL and b.plan == SM.PLAN_TILES and not b.pending
        # the same logical history: generation counter, settings, tracking
        assert (a.generation, a.obj, a.survivors, a.arith, a.waves, a.fb, a.tracking) == \
               (b.generation, b.obj, b.survivors, b.arith, b.waves, b.fb, b.tracking)
        assert [c for c in b.calls if c[0] == "execute_generations"] == []


@pytest.mark.parametrize("shape", SHAPES)
def test_a_cut_list_is_legal_and_ends_in_a_checkpoint(shape):
    for seed in SM.SEEDS[shape][:4]:
        ops, _, boundaries = SM.generate(shape, seed)
        for k in (1, 7, 20, 33, 59):
            head = SM.cut(shape, ops, boundaries, k)
            assert head[:k] == [op for op in ops[:len(head)] if op[0] != "final_lazy"][:k]
            drive(shape, head, "A")
            drive(shape, SM.normalise(head), "B")
            assert head[-1][0] in ("checkpoint", "final_lazy")


@pytest.mark.parametrize("shape", SHAPES)
def test_the_committed_seeds_contain_every_situation(shape):
    """Conditions, not measurements: over the 12 committed seeds every situation a shape can reach occurs at least three
    times, by the generator's own bookkeeping; what a shape cannot reach is named in IMPOSSIBLE, never silently absent."""
    total = {k: 0 for k in SM.SITUATIONS}
    calls = checkpoints = 0
    for seed in SM.SEEDS[shape]:
        ops, stats, _ = SM.generate(shape, seed)
        for k, v in stats.items():
            total[k] += int(v)
        calls += len(ops)
        checkpoints += sum(op[0] == "checkpoint" for op in ops)
    for k, text in SM.SITUATIONS.items():
        if k in SM.IMPOSSIBLE[shape]:
            assert total[k] == 0, (shape, k, text)
        else:
            assert total[k] >= 3, (shape, k, text, total)
    assert checkpoints * 8 <= calls, "checkpoints are drawn with a probability of at most 1 in 8"
    sh = SM.Shape(shape)
    assert (not sh.selection) == (SM.IMPOSSIBLE[shape] != "")


def test_every_kind_of_operation_is_drawn():
    seen = set()
    for shape in SHAPES:
        for seed in SM.SEEDS[shape]:
            seen |= {op[0] for op in SM.generate(shape, seed)[0]}
            seen |= {"refuse:" + op[1] for op in SM.generate(shape, seed)[0] if op[0] == "refuse"}
    want = set(SM.READS) | set(SM.RENDERS) | set(SM.SELECTION) | set(SM.STAGES) | set(SM.LANDSCAPE) | {
        "execute_generations", "execute_generation", "execute_until", "init_population", "write_population", "set_generation",
        "inject_immigrants", "track", "checkpoint", "final_lazy"} | {"refuse:" + r[0] for r in SM.REFUSALS}
    assert want - seen == set()


def test_the_fake_context_objects():
    """the checker itself: what it must refuse or call illegal"""
    sh = SM.Shape("lists")
    f = SM.FakeContext(sh)
    with pytest.raises(SM.Refused):
        f.execute_generations(1)  # no target
    f.set_target_audio(SM.target_audio(sh, 0))
    f.init_population(0)
    f.set_sort_mode(SM.SORT_TOP)
    f.execute_generations(2)
    assert f.pending and not f.tail_defined
    f.read_population()
    assert f.pending  # a pure read keeps the state under TOP_ONLY
    for bad in (f.synthesise, f.sort, f.bucket_fitness, lambda: f.write_population(values=np.zeros((sh.P, sh.D), np.float32))):
        g = SM.FakeContext(sh)
        g.__dict__.update({k: (list(v) if isinstance(v, list) else v) for k, v in f.__dict__.items()})
        with pytest.raises(SM.Illegal):
            getattr(g, bad.__name__)() if bad.__name__ != "<lambda>" else g.write_population(values=np.zeros((sh.P, sh.D), np.float32))
    with pytest.raises(SM.Refused):
        f.pack_elites(sh.S + 1)
    with pytest.raises(SM.Refused):  # refused before anything changes
        f.write_population(values=np.zeros((sh.P - 1, sh.D), np.float32))
    assert f.pending
    f.set_sort_mode(SM.SORT_LAZY)
    assert not f.pending and f.tail_defined
    f.execute_generations(1)
    with pytest.raises(SM.Illegal):
        f.window()  # the fused loop's audio is not the staged loop's
    f.select()
    with pytest.raises(SM.Illegal):
        f.read_population()  # select must be followed by rotate
    f.rotate()
    b = SM.FakeContext(sh, "B")
    with pytest.raises(SM.Illegal):
        b.set_sort_mode(SM.SORT_LAZY)
    with pytest.raises(SM.Illegal):
        b.read_population()


def test_first_difference_compares_bits():
    a = {"x": np.array([[1.0, np.nan], [0.0, 2.0]], np.float32)}
    b = {"x": a["x"].copy()}
    assert SM.first_difference(a, b) is None
    b["x"][1, 0] = -0.0
    assert SM.first_difference(a, b) == ("x", 1)


# ---- the batch's lists ------------------------------------------------------------------------------------------------------
def check_batch_list(shape, ops):
    """the legality of a batch list, kept apart from the generator's own bookkeeping"""
    sh = SM.BatchShape(shape)
    active = made = 0
    track, queue, kept = (False, 0), 0, False
    for op in ops:
        name, a = op[0], op[1:]
        if name in ("set_target_audio", "set_target_spectra"):
            assert 1 <= a[0] <= sh.slots
            made = min(made, a[0]) if a[0] <= active else 0
            active = a[0]
        elif name == "init_population":
            assert active
            made = active
        elif name in ("execute_generations", "execute_until", "read_best", "read_population", "best_ever", "history"):
            assert active and made >= active, (name, "a chunk whose population nobody made since the count grew")
            if name in ("read_population", "history"):
                assert a[0] < active
            if name in ("execute_until", "best_ever"):
                assert track[0]
            if name == "history":
                assert track[1]
        elif name == "track":
            track = (bool(a[0] or a[1]), a[1])
        elif name in ("queue_targets_audio", "queue_targets_spectra"):
            queue, kept = a[0], False
        elif name == "queue_set_carry":
            assert a[0] == 0 or (1 <= a[0] <= sh.parents and a[1] >= 1)
        elif name == "queue_run":
            assert queue and track[0] and not track[1] and a[1] >= 1 and (a[5] is None or a[5] < queue)
            active = made = 0
            kept = a[5] is not None
        elif name == "queue_score_audio_hop":
            assert queue == a[0] and 1 <= a[1] <= sh.N
        elif name == "queue_kept_population":
            assert kept
        elif name == "checkpoint":
            assert a[0] == (active if active and made >= active else 0)
            assert a[1] == track[0] and a[2] == bool(track[0] and track[1])
        elif name == "refuse":
            if a[0] == "execute_generations":
                assert not active
            if a[0] == "queue_run":
                assert not queue or not track[0] or track[1]
            if a[0] == "read_population":
                assert active
        else:
            assert name in ("set_objective", "set_objective_weights", "set_survivors", "set_analysis", "analyse_audio_hop", "getters"), name


@pytest.mark.parametrize("shape", list(SM.BATCH_SHAPES))
def test_batch_lists_are_legal_repeatable_and_cover_their_situations(shape):
    for seed in range(SWEEP):
        ops, _ = SM.generate_batch(shape, seed)
        assert len(ops) == SM.BATCH_OPS and ops[-1][0] == "checkpoint"
        check_batch_list(shape, ops)
    total = {}
    for seed in SM.BATCH_SEEDS[shape]:
        ops, stats = SM.generate_batch(shape, seed)
        assert SM.generate_batch(shape, seed) == (ops, stats)
        for k, v in stats.items():
            total[k] = total.get(k, 0) + int(v)
    # chunk counts that shrink and grow, queue runs with more chunks than slots, with carried rows, with a kept chunk, targets
    # made by the device analysis, refusals, stop rules, a setter between generations: each at least twice in the 8 seeds
    assert all(v >= 2 for v in total.values()), total
