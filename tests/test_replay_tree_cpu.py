"""The inputs of tests/test_replay_tree_gpu.py reach what they are meant to reach (oracle only, no GPU).

A GPU test that compares a descent with the reference's proves something about the LDS / memory hand-over, the second wave
or the second pass of a loop only if its inputs get there.  This file plays the same cases (tests/replay_tree_cases.py) on
the oracle alone and asserts that they do:

  A  every case whose tree has nodes >= 2048 has strata whose descent reads such a node while its kind differs from the
     running mass's kind (the count is printed), and no stratum's mass reaches the tree's total;
  B  every planted stratum meets `left == mass` at the intended heap level, ends on the leftmost leaf of the right
     subtree, and a mass just below it ends on the last leaf of the left subtree;
  C  the update_losses calls re-prioritise the stated numbers of distinct leaves;
  D  for every (rank, Bg) of the global sampler the shard owns some but not all strata, and the halved batch drops some.
  E  at T = 136, 200 and 264 with the leaf the cube of the mean, a pairwise sum split anywhere but where NumPy splits
     moves float32 leaves past their 1-ulp bar.
"""
import functools

import numpy as np
import pytest

from tests import replay_tree_cases as tc
from tests.golden.streams import scalar_kind


def _trace(tree, mass):
    """find_prefixsum_idx step by step -> ([(child read, left, mass before the decision)], leaf slot)."""
    pos, steps = 1, []
    while pos < tree.capacity:
        left = tree.nodes[2 * pos]
        steps.append((2 * pos, left, mass))
        if left > mass:
            pos = 2 * pos
        else:
            mass -= left
            pos = 2 * pos + 1
    return steps, pos - tree.capacity


@functools.lru_cache(maxsize=None)
def _played(name, global_scaling=False):
    """The A sequence of the GPU file on the oracle: feed, then three rounds of (draw at every batch size, update_losses on
    the rows of one of the draws)."""
    _, _, cap, update_B, hist = tc.CASES[name]
    ora = tc.make_oracle(name, global_scaling)
    tc.feed(name, ora)
    assert ora.tree.capacity == cap
    T = hist["nstep_train"]
    mixed_global_reads, draws, sizes = 0, 0, set()
    for rnd in range(tc.ROUNDS):
        active = tc.active_count(ora)
        picked = None
        for B in tc.batch_sizes(name, active):
            us = tc.uniforms(name, rnd, B)
            total = ora.tree.total()
            slots = []
            for mass in tc.stratum_masses(ora.tree, B, us):
                assert mass < total, (name, rnd, B)            # precondition: no stratum walks into the padding
                steps, slot = _trace(ora.tree, mass)
                assert ora.slot_record[slot] is not None       # ... or onto an inactive leaf
                slots.append(slot)
                mixed_global_reads += any(c >= tc.LDS_NODES and scalar_kind(left) != scalar_kind(m) for c, left, m in steps)
            assert np.array_equal(slots, tc.stratified(ora.tree, B, us))
            draws += 1
            sizes.add(B)
            if B == update_B:
                picked = slots
        se, sb = tc.oracle_slot_table(ora)
        rows = tc.sequence_rows(picked, se, sb, T)
        ora.update_losses(rows, tc.losses(name, rnd, len(rows)))
    return {"ora": ora, "mixed_global_reads": mixed_global_reads, "draws": draws, "sizes": sizes}


@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_a_streams_cross_the_staging_boundary_with_mixed_kinds(name):
    got = _played(name)
    cap = tc.CASES[name][2]
    print("%s: capacity %d, %d draws, strata reading a node >= %d of another kind than their mass: %d"
          % (name, cap, got["draws"], tc.LDS_NODES, got["mixed_global_reads"]))
    if 2 * cap > tc.LDS_NODES:
        assert got["mixed_global_reads"] > 0
    else:
        assert got["mixed_global_reads"] == 0 and name == "t1_1000"     # the all-staged control
    want = {1000: 4, 2000: 7, 3000: 8, 5000: 8}[tc.CASES[name][4]["size"]] if name.startswith("t1") else 8
    assert len(got["sizes"]) == want                                  # every batch size the active count allows was drawn


def test_a_sequence_tree_holds_all_four_scalar_types():
    """T = 8, overlap 7, 3200 transitions into 3000: updated np.float32, fresh np.float64, never-used Python float 0.0
    and evicted Python int 0 leaves in one tree."""
    ora = _played("t8_3000")["ora"]
    leaves = ora.tree.nodes[ora.tree.capacity:]
    assert {type(x) for x in leaves} == {float, int, np.float32, np.float64}
    print({t.__name__: sum(type(x) is t for x in leaves) for t in (float, int, np.float32, np.float64)})


def _planted_tree(pattern):
    ora = tc.make_oracle(tc.PLANT_CASE)
    tc.feed(tc.PLANT_CASE, ora)
    cap = ora.tree.capacity
    leaves = ora.tree.nodes[cap:]
    assert all(type(x) is float and x == 1.0 for x in leaves[:5000]) and all(x == 0.0 for x in leaves[5000:])
    v = np.array([float(x) for x in leaves])
    k = np.zeros(cap, dtype=np.uint8)
    v[:tc.PLANT_N], k[:tc.PLANT_N] = tc.planted_leaves(pattern)
    return tc.load_tree(v, k)


@pytest.mark.parametrize("pattern", tc.PLANT_PATTERNS)
def test_b_planted_strata_tie_at_their_level(pattern):
    tree = _planted_tree(pattern)
    v, k = tc.planted_leaves(pattern)
    assert float(tree.total()) == tc.PLANT_TOTAL
    assert scalar_kind(tree.total()) == {"weak": 0, "f32": 1, "mixed": 2, "f32_offgrid": 1}[pattern]
    if pattern == "mixed":
        assert all(len(set(k[b:b + 64])) > 1 for b in range(0, tc.PLANT_N, 64))
    us, ties = tc.planted_uniforms()
    assert us.max() <= 1.0 - 2.0 ** -10 and np.array_equal(us * 16, np.round(us * 16))
    assert len({i for _, _, i in ties}) == len(ties) and {lvl for lvl, _, _ in ties} == set(tc.TIE_LEVELS)
    masses = tc.stratum_masses(tree, tc.PLANT_B, us)
    assert all(m < tree.total() for m in masses)
    slots = tc.stratified(tree, tc.PLANT_B, us)
    for lvl, b, i in ties:
        steps, slot = _trace(tree, masses[i])
        tied = [c for c, left, m in steps if left == m]
        assert tied and tied[0].bit_length() - 1 == lvl and tied[0] % 2 == 0, (pattern, lvl, b)
        assert slot == b == slots[i]
        # A mass just below the boundary stays in the left subtree.  (One float64 ulp of u itself is absorbed by the
        # addition of i * seg for every stratum but the first, so the mass is moved: by one ulp of its own type, and by
        # a sixteenth, the smallest step of u that survives the float32 form at this magnitude.)
        m = masses[i]
        below = type(m)(np.nextafter(m, type(m)(0)))
        assert type(below) is type(m) and below < m
        assert _trace(tree, below)[1] == b - 1
        moved = tc.stratum_masses(tree, tc.PLANT_B, np.where(np.arange(tc.PLANT_B) == i, us - 2.0 ** -8, us))[i]
        assert moved < m and _trace(tree, moved)[1] == b - 1
    if pattern == "f32_offgrid":
        # the level-13 ties are decided by the float32 cast of the weak leaf: in exact arithmetic the leaf is greater
        for lvl, b, i in ties:
            if lvl == 13:
                left = tree.nodes[tree.capacity + b - 1]
                steps, _ = _trace(tree, masses[i])
                assert type(left) is float and float(left) > float(steps[-1][2]) and not left > steps[-1][2]


def test_c_update_calls_touch_the_stated_numbers_of_leaves():
    ora = tc.make_oracle(tc.FIX_CASE)
    tc.feed(tc.FIX_CASE, ora)
    touched = []
    inner = ora._reprioritize
    ora._reprioritize = lambda slot: (touched.append(slot), inner(slot))[1]
    seen = []
    for rows, ls, distinct in tc.fix_calls(ora):
        del touched[:]
        ora.update_losses(rows, ls)
        assert len(touched) == len(set(touched)) == distinct
        seen.append(distinct)
    assert seen == [1023, 1024, 1025, 2049, 600]
    rows, ls, _ = tc.fix_calls(ora)[-1]
    assert np.array_equal(rows[600:], rows[:300]) and not np.any(ls[600:] == ls[:300])
    for (env, off), want in zip(rows[:300], ls[600:]):              # the later row won
        assert ora.rings[env][off - ora.env_first_offset[env]]["loss"] == abs(want) + ora.eps


def test_d_every_rank_owns_some_strata_and_the_halved_batch_drops():
    ora = tc.make_oracle(tc.GLOBAL_CASE)
    tc.feed(tc.GLOBAL_CASE, ora)
    tc.prepare_global(ora)
    kinds = {scalar_kind(x) for x in ora.tree.nodes[ora.tree.capacity:] if x != 0}
    assert kinds == {1, 2}
    total, active, beta = float(ora.tree.total()), tc.active_count(ora), ora.beta
    plan = tc.global_plan()
    assert [c for c, _, _ in plan] == list(range(1, 13))
    for call, rank, Bg in plan + [(len(plan) + 1,) + tc.GLOBAL_DROP]:
        want = tc.global_expected(ora.tree, tc.shard_table(rank, total, active), rank, Bg, call, beta)
        owned = len(want["stratum"])
        assert 0 < owned < Bg, (rank, Bg)
        assert np.all(want["local_mass"] < total) and np.all(want["local_mass"] >= 0)
        assert all(ora.slot_record[s] is not None for s in want["slot"])
        print("call %d rank %d Bg %d: owns %d" % (call, rank, Bg, owned))
    assert owned // 2 >= 1 and owned - owned // 2 >= 1                 # the last entry is the halved-rows repeat


@pytest.mark.parametrize("T", tc.LONG_T)
def test_e_a_wrong_split_point_moves_a_leaf_by_more_than_its_bar(T):
    """At max_weight_factor 0 and alpha 3 the leaf is (mean of the T losses) ** 3.  For the loss vectors of the GPU test:
    the restated pairwise sum equals np.add.reduce bit for bit and gives the oracle's leaf; the same sum split at n // 2
    without the rounding to a multiple of 8 moves at least one float32 leaf past the 1-ulp bar."""
    from oracle import replay as orc
    from tests.golden.streams import vector_steps, as_reference_samples
    ora = orc.OraclePrioritizedReplay(**tc.long_hist(T), discount_function=orc.make_discount(tc.GAMMA))
    spec, step = tc.long_spec(T), 0
    caught = {np.float32: 0, np.float64: 0}
    for feed_steps, rows, ls in tc.long_rounds(T):
        for st in vector_steps(spec, feed_steps, start_step=step):
            ora.update(as_reference_samples(spec, st))
        step += feed_steps
        touched = []
        inner = ora._reprioritize
        ora._reprioritize = lambda slot: (touched.append(slot), inner(slot))[1]
        ora.update_losses(rows, ls)
        ora._reprioritize = inner
        assert len(ora.free_slots) == ora.n_slots - tc.active_count(ora) and len(ora.fifo) < ora.size      # nothing evicted
        for slot in touched:
            head = ora.slot_record[slot]
            pos = head["env_buffer_offset"] - ora.env_first_offset[head["env_id"]]
            a = np.array([rec["loss"] for rec in ora.rings[head["env_id"]][pos:pos + T]])
            assert len(a) == T and a.dtype in (np.float32, np.float64)      # np.float64 once a fresh Python float is in the list
            good, bad = tc.np_pairwise_sum(a, 0, T), tc.np_pairwise_sum(a, 0, T, round_split=False)
            assert good == np.add.reduce(a) and type(good) is a.dtype.type
            leaf = lambda s: (0.0 * np.max(a) + (1 - 0.0) * a.dtype.type(s / T)) ** 3.0                      # noqa: E731
            want = ora.tree.leaf(slot)
            assert leaf(good) == want and type(leaf(good)) is type(want)
            bar = 1.3e-7 if a.dtype == np.float32 else 4.5e-16                                             # scenario.check_leaf_values
            caught[a.dtype.type] += abs(float(leaf(bad)) - float(want)) > bar * float(want)
    print("T = %d: leaves a wrong split point moves past the bar: %d float32, %d float64" % (T, caught[np.float32], caught[np.float64]))
    # a float64 sum of at most 264 float32 numbers of this range is exact, so no order of additions can show there
    assert caught[np.float32] > 0 and caught[np.float64] == 0
