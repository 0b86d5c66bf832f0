"""The variation model of tests/_variation_model.py against the CPU oracle, its power over the geometries the GPU test
runs, and the branch coverage of every population the GPU test writes (tests/test_gpu_variation.py).  No GPU."""
import numpy as np
import pytest

import _variation_model as vm

DIMS = {0: 4, 1: 6, 2: 12, 3: 8}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def numbered(p, d):
    """every gene its own number (exact in fp32 below 2^24), steps likewise and different from the values"""
    v = np.arange(p * d, dtype=np.float32).reshape(p, d)
    return v, v + np.float32(0.5)


# ---- recombination ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,parents,block", [
    (300, 9, 1), (300, 9, 3), (288, 72, 24), (288, 20, 24), (288, 24, 24), (288, 100, 24), (256, 96, 32), (288, 48, 48), (384, 150, 48),
    (384, 96, 96), (576, 300, 96), (400, 100, 100), (900, 520, 100), (300, 77, 300), (576, 64, 576), (256, 64, 256)])
@pytest.mark.parametrize("d", [4, 6, 12, 8])
def test_model_recombine_equals_the_oracle(O, p, parents, block, d):
    """blocks 1, 3, 24, 32, 48, 96, 100 and B = P; parents below, equal to and not a multiple of the block"""
    rng = np.random.default_rng(p + block)
    v, s = rng.random((p, d), dtype=np.float32), rng.random((p, d), dtype=np.float32)
    mv, ms = vm.recombine(v, s, parents, block)
    ov, os_ = O.recombine(v, s, parents, block)
    assert np.array_equal(bits(mv), bits(ov)) and np.array_equal(bits(ms), bits(os_))


@pytest.mark.parametrize("kind,parents,offspring,block", vm.GEOMETRIES[:-1])
def test_model_recombine_equals_the_oracle_at_the_gpu_geometries(O, kind, parents, offspring, block):
    v, s = numbered(parents + offspring, DIMS[kind])
    mv, ms = vm.recombine(v, s, parents, block)
    ov, os_ = O.recombine(v, s, parents, block)
    assert np.array_equal(bits(mv), bits(ov)) and np.array_equal(bits(ms), bits(os_))


def test_gpu_geometries_are_what_the_issue_lists():
    blocks = {g[3] for g in vm.GEOMETRIES}
    assert {3, 24, 48, 96, 100} <= blocks and any(g[3] == g[1] + g[2] for g in vm.GEOMETRIES)
    assert {g[0] for g in vm.GEOMETRIES} == {0, 1, 2, 3}
    b24 = [g for g in vm.GEOMETRIES if g[3] == 24]
    assert any(g[1] < 24 for g in b24) and any(g[1] == 24 for g in b24) and any(g[1] > 24 and g[1] % 24 for g in b24)
    assert {3, 5, 9} <= {g[1] // g[3] for g in vm.GEOMETRIES}
    kind, parents, offspring, block = vm.GEOMETRIES[-1]
    assert block == 24 and (parents + offspring) * DIMS[kind] > 2048 * 256, "the last geometry wraps the grid-stride loop"
    for _, parents, offspring, block in vm.GEOMETRIES:
        assert (parents + offspring) % block == 0


# ---- power: a wrong kernel must move a gene in at least one geometry of the GPU list -------------------------------------------
def gather(p, d, parents, block, fault=None):
    """the KERNEL's form (a gather), with one fault: source element of every (row, gene), or -1 where it leaves the population"""
    i = np.arange(p, dtype=np.int64)[:, None]
    g = np.arange(d, dtype=np.int64)[None, :]
    npb = max(1, parents // block)
    b, dl = i // block, i % block
    if fault == "modulus B - 1":
        l = (dl - g * (b + 1)) % max(1, block - 1)
    elif fault == "b for b + 1":
        l = (dl - g * b) % block
    elif fault == "shift before multiply":
        # (g (b + 1)) mod B taken as g ((b + 1) mod B): the 32-bit difference dl + B - shift then wraps below zero, which a
        # power-of-two block forgives (2^32 is a multiple of it) and no other block does
        l = ((dl + block - g * ((b + 1) % block)) % (1 << 32)) % block
    else:
        l = (dl - g * (b + 1)) % block
    pb = b % (npb + 1) if fault == "parent block b % (npb + 1)" else b % npb
    row = pb * block + l
    return np.where(row < p, row * d + g, -1)


FAULTS = ["modulus B - 1", "b for b + 1", "parent block b % (npb + 1)", "shift before multiply"]


def model_map(p, d, parents, block):
    v, s = numbered(p, d)
    mv, _ = vm.recombine(v, s, parents, block)
    return mv.astype(np.int64)


def test_the_faultless_gather_is_the_model():
    for kind, parents, offspring, block in vm.GEOMETRIES:
        p, d = parents + offspring, DIMS[kind]
        assert np.array_equal(gather(p, d, parents, block), model_map(p, d, parents, block)), (kind, parents, offspring, block)


@pytest.mark.parametrize("fault", FAULTS)
def test_a_wrong_recombination_is_caught_by_a_gpu_geometry(fault):
    caught = []
    for kind, parents, offspring, block in vm.GEOMETRIES:
        p, d = parents + offspring, DIMS[kind]
        if not np.array_equal(gather(p, d, parents, block, fault), model_map(p, d, parents, block)):
            caught.append((kind, parents, offspring, block))
    print(fault, "caught by", len(caught), "of", len(vm.GEOMETRIES))
    assert caught, fault
    if fault == "shift before multiply":
        assert all(block & (block - 1) for _, _, _, block in caught), "only a block that is no power of two shows this fault"


@pytest.mark.parametrize("fault", FAULTS)
def test_a_wrong_recombination_is_caught_at_the_site_shape(fault):
    """block 24, 80 parents (3 parent blocks), the smallest site population"""
    p = min(s[2] for s in vm.SITES)
    assert not np.array_equal(gather(p, 4, vm.SITE_PARENTS, vm.SITE_BLOCK, fault), model_map(p, 4, vm.SITE_PARENTS, vm.SITE_BLOCK))


# ---- mutation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("generation", [5, 0xFFFFFFFF])
def test_model_mutate_equals_the_oracle_on_the_edge_population(O, kind, generation):
    """values bit for bit (a NaN for a NaN); steps within the GPU test's bound of the oracle's libm steps"""
    d = DIMS[kind]
    v, s = vm.edge_population(d)
    words = O.mutate_words(v.shape[0], d, vm.SEED, 77, generation)
    mv, ms = vm.mutate(v, s, words, d)
    ov, os_ = O.mutate(v, s, vm.SEED, 77, generation)
    assert vm.same_values(mv, ov)
    assert np.array_equal(np.isnan(mv), np.isnan(ov))
    ratio = vm.step_ratio(os_, ms)
    print("oracle steps against the model, worst ratio", float(ratio.max()))
    assert np.all(ratio <= 1.0), (int(np.argmax(ratio)), float(ratio.max()))
    # IEEE leaves no choice: from the model's result, not from constants
    for mask in (ms == 0.0, np.isinf(ms), np.isnan(ms)):
        assert mask.any()
    assert np.array_equal(ms == 0.0, s == 0.0) and np.array_equal(np.isnan(ms), np.isnan(s)) and np.array_equal(np.isinf(ms), np.isinf(s))


def test_model_mutate_equals_mutate_gene_word_by_word(O):
    d = 6
    v, s = vm.edge_population(d, rows=96)
    words = O.mutate_words(96, d, vm.SEED, 0, 1)
    assert words[3, 2, 7] == O.draw_word(vm.SEED, 3, 1, 2 * 16 + 7)
    mv, ms = vm.mutate(v, s, words, d)
    for i in range(96):
        for j in range(d):
            gv, gs = O.mutate_gene(v[i, j], s[i, j], d, words[i, j])
            assert vm.same_values(mv[i, j], gv)
            assert vm.step_ratio(gs, ms[i, j]) <= 1.0


def test_step_ratio_judges():
    big = np.float64(3.4029e38)   # FLT_MAX is 3.40282e38
    assert vm.step_ratio(np.float32(np.inf), big) == 0.0          # rounds to inf in fp32
    assert vm.step_ratio(np.float32(np.inf), big * 0.99) == np.inf         # cannot
    assert vm.step_ratio(np.float32(3.0e38), np.float64(3.0e38)) <= 1.0
    assert vm.step_ratio(np.float32(0.0), np.float64(2.0 ** -150)) <= 1.0  # rounds into the subnormals
    assert vm.step_ratio(np.float32(1.0), np.float64(1.0 + 3e-6)) > 1.0
    assert vm.step_ratio(np.float32(np.nan), np.float64(np.nan)) == 0.0 and vm.step_ratio(np.float32(1.0), np.float64(np.nan)) == np.inf
    assert vm.step_ratio(np.float32(1e-45), np.float64(0.0)) == np.inf and vm.step_ratio(np.float32(np.nan), np.float64(1.0)) == np.inf


def test_survivors_are_bit_copies():
    v0, s0 = numbered(8, 4)
    v1, s1 = vm.survivors(v0, s0, v0 + 100, s0 + 100, 3)
    assert np.array_equal(v1[:3], v0[:3]) and np.array_equal(s1[:3], s0[:3]) and np.array_equal(v1[3:], v0[3:] + 100)


def test_init_equals_the_oracle(O):
    p, d = 48, 6
    for gid, chunk in ((0, 0), (vm.WRAP_GID, vm.EDGE_CHUNK)):
        words = np.array([[O.draw_word(vm.SEED, gid + i, chunk, j, O.TAG_INIT) for j in range(d)] for i in range(p)], np.uint32)
        v, s = vm.init(words)
        ov, os_ = O.init_population(p, d, vm.SEED, gid & 0xFFFFFFFF, chunk)
        assert np.array_equal(bits(v), bits(ov)) and np.array_equal(bits(s), bits(os_))


# ---- coverage of every population the GPU test writes ---------------------------------------------------------------------------
def written_populations(O):
    """(name, values, steps, words, d) of every population tests/test_gpu_variation.py mutates, as mutation meets it"""
    for kind in range(4):
        d = DIMS[kind]
        v, s = vm.edge_population(d)
        for gen in (vm.SITE_GENERATION,) + vm.EDGE_GENERATIONS:
            yield f"edge voice {kind} generation {gen}", v, s, O.mutate_words(v.shape[0], d, vm.SEED, 0, gen), d
    for name, kind, p, _ in vm.SITES:
        d = DIMS[kind]
        words = O.mutate_words(p, d, vm.SEED, 0, vm.SITE_GENERATION)
        v, s = vm.site_population(p, d, p + kind)
        yield (name,) + vm.recombine(v, s, vm.SITE_PARENTS, vm.SITE_BLOCK) + (words, d)
        v, s = vm.edge_population(d, finite=True, rows=p)
        yield (name + " finite edges",) + vm.recombine(v, s, vm.SITE_PARENTS, vm.SITE_BLOCK) + (words, d)
    v, s = vm.site_population(vm.WRAP_P, 4, 99)
    rv, rs = vm.recombine(v, s, vm.SITE_PARENTS, vm.SITE_BLOCK)
    for gen in (vm.SITE_GENERATION,) + vm.EDGE_GENERATIONS:
        yield f"wrapping gid_base, generation {gen}", rv, rs, O.mutate_words(vm.WRAP_P, 4, vm.SEED, vm.WRAP_GID, gen), 4


def test_every_written_population_takes_every_branch(O):
    worst = [1.0] * 5
    for name, v, s, words, d in written_populations(O):
        c = vm.coverage(v, s, words, d)
        worst = [min(a, b) for a, b in zip(worst, c)]
        assert c[0] >= 0.25 and c[1] >= 0.25, (name, "coin", c)
        assert c[2] >= 0.10, (name, "reflect taken", c)
        assert c[3] >= 0.10, (name, "reflect not taken", c)
        assert c[4] >= 0.05, (name, "still outside after the reflection", c)
    print("smallest shares (coin even, odd, reflect taken, not taken, still outside of reflected):", [round(x, 3) for x in worst])
