"""The PER sampler and tree kernels past their single-pass sizes, against the reference's tree (csrc/replay.hip:
k_per_sample, k_per_sample_global, k_tree_fix, k_recalc_flagged / k_recalc_flagged_wave; csrc/np_emul.h).

Both samplers keep heap nodes [0, 2048) in LDS and read every child >= 2048 from memory, loop `i += 1024` over the strata
and combine 16 per-wave partials; k_tree_fix loops `i += 1024` over the dirty leaves.  Here trees of capacity 2048, 4096 and
8192 are drawn from at B up to 3000, and up to 2049 leaves are dirty in one call.

How expected values are formed: the expected tree is the oracle tree (oracle/sumtree.py) REBUILT FROM THE DEVICE'S OWN LEAVES,
values and kinds as tree_nodes() reads them back.  Inner nodes, sampled slots and the min tree are then compared bit for bit,
without inheriting the 1-ulp `pow` difference of a leaf value; that difference is bounded separately, against
OraclePrioritizedReplay run on the same stream (scenario.check_leaf_values), together with leaf kinds and the free list.
Importance weights: scenario.WEIGHT_RTOL of the reference's expression on its own scalars, the project's bar for this
quantity; stats[1], the normaliser, is itself such a weight and is held to the same bar, stats[0] (the root) exactly.  The
global sampler's raw weight: 2^-50 relative (4 ulp of float64) — the operand of pow is the same IEEE sequence on both sides
and the two pow implementations are each within 1 ulp.

tests/test_replay_tree_cpu.py proves on the oracle alone that these inputs reach the memory levels with mixed kinds, tie where
they are planted to tie, dirty the stated numbers of leaves and split every global batch between the ranks.
"""
import numpy as np
import pytest
import torch

from oracle.sumtree import MinTree
from tests import replay_tree_cases as tc
from tests import scenario
from tests.golden.streams import scalar_kind

pytestmark = pytest.mark.gpu

GUARD = 64
PROGRESS = 0.5


def _make(name, global_scaling=False):
    from rltime_amd.history import PrioritizedReplayHistoryBuffer
    ora = tc.make_oracle(name, global_scaling)
    dev = PrioritizedReplayHistoryBuffer(**tc.hist_of(name, global_scaling), gamma=tc.GAMMA)
    tc.feed(name, ora, dev)
    return ora, dev


def _check_tree(dev, ora, tag):
    """After a feed or an update: every inner node, value and kind, equals the tree rebuilt from the device's leaves; the
    leaves equal the oracle replay's in kind and within 1 ulp; free list and slot table equal the oracle's; with a min tree,
    the same for it.  -> (sum tree, min tree or None) of the reference's scalars, loaded from the device's leaves."""
    v, k, m = dev.tree_nodes()
    cap = len(v) // 2
    assert cap == ora.tree.capacity
    tree = tc.load_tree(v[cap:], k[cap:])
    wv, wk = tc.tree_arrays(tree)
    assert np.array_equal(k[1:], wk[1:]), tag
    bad = np.flatnonzero(v[1:] != wv[1:]) + 1
    assert bad.size == 0, "%s: %d inner nodes differ from the rebuild, first %s" % (tag, bad.size, bad[:8])
    ora_v = np.array([float(x) for x in ora.tree.nodes[cap:]])
    ora_k = np.array([scalar_kind(x) for x in ora.tree.nodes[cap:]], dtype=np.uint8)
    assert np.array_equal(k[cap:], ora_k), tag
    scenario.check_leaf_values(v[cap:], ora_v, ora_k, tag, False)
    assert np.array_equal(dev.free_slots(), np.array(list(ora.free_slots))), tag
    se, sb = dev.slot_table()
    ose, osb = tc.oracle_slot_table(ora)
    assert np.array_equal(se, ose) and np.array_equal(sb, osb), tag
    mtree = None
    if ora.min_tree is not None:
        live = np.zeros(cap, dtype=bool)
        live[:len(se)] = se >= 0
        assert np.array_equal(m[cap:], np.where(live, v[cap:], np.inf)), tag
        mtree = tc.load_tree(m[cap:], k[cap:], cls=MinTree)
        assert np.array_equal(m[1:], tc.tree_arrays(mtree)[0][1:]), tag
        ora_m = np.array([float(x) for x in ora.min_tree.nodes[cap:]])
        scenario.check_leaf_values(m[cap:], ora_m, ora_k, tag + " min", False)
    return tree, mtree


def _guarded(n, dtype, fill):
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")


def _head(t, n, tag):
    """The first n elements; the guard tail behind them must still hold its fill."""
    a = t.cpu().numpy()
    tail = a[n:]
    assert len(tail) == GUARD and (np.isnan(tail).all() if a.dtype.kind == "f" else (tail == -7).all()), tag + ": guard tail written"
    return a[:n]


def _draw(dev, ora, tree, mtree, B, us, tag):
    """One mirl_replay_sample call (k_per_sample) on host uniforms -> the slots, after every output was compared."""
    from rltime_amd._lib import lib, check, np_ptr, ptr, stream
    slot, env = _guarded(B, torch.int32, -7), _guarded(B, torch.int32, -7)
    start, base = _guarded(B, torch.int64, -7), _guarded(B, torch.int64, -7)
    weight, stats = _guarded(B, torch.float32, float("nan")), _guarded(2, torch.float64, float("nan"))
    us = np.ascontiguousarray(us, dtype=np.float64)
    rc = check(lib.mirl_replay_sample(dev._h, B, PROGRESS, np_ptr(us), 1, ptr(slot), ptr(env), ptr(start), ptr(base),
                                      ptr(weight), ptr(stats), stream()), "mirl_replay_sample")
    assert rc == 0, tag
    torch.cuda.synchronize()
    want = tc.stratified(tree, B, us)
    got = _head(slot, B, tag).astype(np.int64)
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, "%s: %d of %d slots differ, first strata %s: got %s want %s" % (tag, diff.size, B, diff[:6], got[diff[:6]], want[diff[:6]])
    se, sb = tc.oracle_slot_table(ora)
    assert np.array_equal(_head(env, B, tag), se[want]), tag
    assert np.array_equal(_head(start, B, tag), sb[want] - ora.prefix_steps), tag
    assert np.array_equal(_head(base, B, tag), sb[want]), tag
    w, top = tc.weights(tree, want, tc.active_count(ora), ora.beta, mtree)
    np.testing.assert_allclose(_head(weight, B, tag), w.astype(np.float32), rtol=scenario.WEIGHT_RTOL, atol=0, err_msg=tag)
    st = _head(stats, 2, tag)
    assert st[0] == float(tree.total()), tag
    np.testing.assert_allclose(st[1], float(top), rtol=scenario.WEIGHT_RTOL, atol=0, err_msg=tag)
    return want


# ----------------------------------------------------------------------------------------------------------------------
# A. descent across the staging boundary, reference streams
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,global_scaling", [(n, False) for n in sorted(tc.CASES)] + [(n, True) for n in tc.GLOBAL_SCALING_CASES])
def test_a_stream_draws_and_updates_vs_reference_tree(name, global_scaling):
    """Feed, then three rounds of: draw at every batch size of {1, 63, 64, 65, 1023, 1024, 1025, 3000} the active count
    allows (slots, env, start, weights, stats), update_losses on the rows of one draw (whole tree, leaves, free list; with
    global_importance_scaling the min tree and the p_min form of the weights).  Capacity 1024 is the all-LDS control, at
    2048 the leaf level is read from memory, at 8192 two inner levels are too; T = 8 runs the wave recalc kernel with
    evicted `int` zeros beside fresh np.float64 leaves, T = 4 the lane kernel."""
    ora, dev = _make(name, global_scaling)
    update_B, T = tc.CASES[name][3], ora.nstep_train
    tree, mtree = _check_tree(dev, ora, name + " fed")
    for rnd in range(tc.ROUNDS):
        picked = None
        for B in tc.batch_sizes(name, tc.active_count(ora)):
            slots = _draw(dev, ora, tree, mtree, B, tc.uniforms(name, rnd, B), "%s round %d B %d" % (name, rnd, B))
            if B == update_B:
                picked = slots
        se, sb = dev.slot_table()
        rows = tc.sequence_rows(picked, se, sb, T)
        ls = tc.losses(name, rnd, len(rows))
        ora.update_losses(rows, ls)
        dev.update_losses(rows, ls)
        tree, mtree = _check_tree(dev, ora, "%s update %d" % (name, rnd))
    dev.close()


# ----------------------------------------------------------------------------------------------------------------------
# B. planted ties on both sides of the hand-over
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plant_shard():
    ora, dev = _make(tc.PLANT_CASE)
    yield ora, dev
    dev.close()


@pytest.mark.parametrize("pattern", tc.PLANT_PATTERNS)
def test_b_planted_ties_go_right_on_both_sides_of_the_hand_over(plant_shard, pattern):
    """Leaves [0, 4096) of the full 5000-slot shard overwritten with small integers (all Python floats, all np.float32, a
    mixture of the three kinds, and np.float32 with weak leaves that are no float32 numbers), B = 1024 with dyadic
    uniforms: selected strata land EXACTLY on the prefix sum at a node boundary of heap levels 9, 10 (staged), 11, 12
    and 13 (memory).  The reference goes right on `left == mass`: the slot is the leftmost leaf of the right subtree."""
    from rltime_amd._lib import lib, check, np_ptr
    ora, dev = plant_shard
    se, _ = dev.slot_table()
    assert len(se) == 5000 and np.all(se[:tc.PLANT_N] >= 0)
    v, k = tc.planted_leaves(pattern)
    v, k = np.ascontiguousarray(v), np.ascontiguousarray(k)
    check(lib.mirl_replay_tree_set_leaves(dev._h, tc.PLANT_N, np_ptr(v), np_ptr(k), None), "mirl_replay_tree_set_leaves")
    dv, dk, _ = dev.tree_nodes()
    cap = len(dv) // 2
    assert np.array_equal(dv[cap:cap + tc.PLANT_N], v) and np.array_equal(dk[cap:cap + tc.PLANT_N], k)
    assert np.all(dv[cap + tc.PLANT_N:cap + 5000] == 1.0) and np.all(dk[cap + tc.PLANT_N:] == 0)
    tree = tc.load_tree(dv[cap:], dk[cap:])
    wv, wk = tc.tree_arrays(tree)
    assert np.array_equal(dv[1:], wv[1:]) and np.array_equal(dk[1:], wk[1:])
    assert dv[1] == tc.PLANT_TOTAL
    us, ties = tc.planted_uniforms()
    slots = _draw(dev, ora, tree, None, tc.PLANT_B, us, "planted " + pattern)
    for lvl, b, i in ties:
        assert slots[i] == b, (pattern, lvl)


# ----------------------------------------------------------------------------------------------------------------------
# C. k_tree_fix past one pass
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("global_scaling", [False, True])
def test_c_tree_fix_with_more_dirty_leaves_than_lanes(global_scaling):
    """update_losses naming 1023, 1024, 1025 and 2049 distinct live transitions of the T = 1 shard (one dirty leaf each),
    then 600 distinct ones of which 300 are repeated two 256-row blocks later with other losses (the last row wins): after
    each call the WHOLE sum tree, and with global scaling the whole min tree, equals the rebuild from the leaves."""
    ora, dev = _make(tc.FIX_CASE, global_scaling)
    for j, (rows, ls, distinct) in enumerate(tc.fix_calls(ora)):
        ora.update_losses(rows, ls)
        dev.update_losses(rows, ls)
        _check_tree(dev, ora, "fix call %d (%d distinct)" % (j, distinct))
    dev.close()


# ----------------------------------------------------------------------------------------------------------------------
# D. k_per_sample_global in one process
# ----------------------------------------------------------------------------------------------------------------------
def _global_call(dev, ora, tree, rank, Bg, rows, call, root, tag):
    from rltime_amd._lib import lib, check, ptr, stream
    shard = torch.from_numpy(tc.shard_table(rank, 0.0, 0.0)).cuda()
    shard[rank] = root                                   # this tree's own {root, active}, as mirl_replay_tree_root wrote it
    shard_host = shard.cpu().numpy()
    slot, env, stratum = (_guarded(rows, torch.int32, -7) for _ in range(3))
    start, base = _guarded(rows, torch.int64, -7), _guarded(rows, torch.int64, -7)
    raw, stats = _guarded(rows, torch.float64, float("nan")), _guarded(4, torch.float64, float("nan"))
    rc = check(lib.mirl_replay_sample_global(dev._h, 1, Bg, rows, rank, 3, ptr(shard), PROGRESS, tc.GLOBAL_SEED, ptr(slot), ptr(env),
                                             ptr(start), ptr(base), ptr(raw), ptr(stratum), ptr(stats), stream()),
               "mirl_replay_sample_global")
    assert rc == 0, tag
    torch.cuda.synchronize()
    want = tc.global_expected(tree, shard_host, rank, Bg, call, ora.beta)
    owned = len(want["stratum"])
    kept = min(owned, rows)
    se, sb = tc.oracle_slot_table(ora)
    ws = want["slot"][:kept]
    got = {"stratum": _head(stratum, rows, tag), "slot": _head(slot, rows, tag), "env": _head(env, rows, tag),
           "start": _head(start, rows, tag), "base": _head(base, rows, tag), "raw": _head(raw, rows, tag)}
    assert np.array_equal(got["stratum"][:kept], want["stratum"][:kept]), tag
    assert np.array_equal(got["slot"][:kept], ws), tag
    assert np.array_equal(got["env"][:kept], se[ws]) and np.array_equal(got["start"][:kept], sb[ws] - ora.prefix_steps), tag
    assert np.array_equal(got["base"][:kept], sb[ws]), tag
    wr = want["raw"][:kept]
    assert np.all(np.abs(got["raw"][:kept] - wr) <= 2.0 ** -50 * wr), tag
    for key, pad in (("stratum", -1), ("slot", -1), ("env", -1), ("start", 0), ("base", 0), ("raw", 0.0)):
        assert np.all(got[key][kept:] == pad), (tag, key)
    st = _head(stats, 4, tag)
    assert st[0] == want["Pg"] and st[2] == kept and st[3] == owned - kept, (tag, st)
    assert abs(st[1] - wr.max()) <= 2.0 ** -50 * wr.max(), tag
    return owned, kept


def test_d_global_sampler_owned_strata_weights_padding_and_drops():
    """One shard of three (the other two rows of the table are fabricated totals), as rank 0, 1 and 2, at Bg = 8, 65, 1025
    and 3000 (more than one pass of both loops, the count across all 16 waves): the owned strata in stratum order with
    slot, env, start and raw weight, padding rows, stats = {P_g, local max, kept, 0}.  Then one rank again with `rows` at
    half its owned count: exactly the first `rows` owned strata, the rest counted in stats[3], nothing written past `rows`."""
    from rltime_amd._lib import lib, check, ptr, stream
    ora, dev = _make(tc.GLOBAL_CASE)
    tc.prepare_global(ora, dev)
    tree, _ = _check_tree(dev, ora, "global prepared")
    root = torch.empty(2, dtype=torch.float64, device="cuda")
    check(lib.mirl_replay_tree_root(dev._h, ptr(root), stream()), "mirl_replay_tree_root")
    own = root.cpu().numpy()
    assert own[0] == float(tree.total()) and own[1] == tc.active_count(ora)
    for call, rank, Bg in tc.global_plan():
        owned, kept = _global_call(dev, ora, tree, rank, Bg, Bg, call, root, "rank %d Bg %d" % (rank, Bg))
        assert 0 < owned == kept < Bg
    rank, Bg = tc.GLOBAL_DROP
    want = tc.global_expected(tree, tc.shard_table(rank, own[0], own[1]), rank, Bg, call + 1, ora.beta)
    rows = len(want["stratum"]) // 2
    owned, kept = _global_call(dev, ora, tree, rank, Bg, rows, call + 1, root, "rank %d Bg %d rows %d" % (rank, Bg, rows))
    assert kept == rows and owned - kept == len(want["stratum"]) - rows > 0
    dev.close()


# ----------------------------------------------------------------------------------------------------------------------
# E. the lane recalc kernel above the wave kernel's range, with the order of its additions visible
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", tc.LONG_T)
def test_e_long_sequence_mean_follows_numpys_pairwise_order(T):
    """k_recalc_flagged at T = 136, 200 and 264 (np_pairwise_sum's explicit stack on the device) with max_weight_factor 0
    and alpha 3: the leaf is the cube of the mean, so a sum one ulp off — any split point but NumPy's — moves it by
    three ulps, past the 1-ulp bar of a leaf (the CPU file counts the leaves that would move).  Fully updated sequences
    (float32 form), then sequences that hold updated losses beside fresh Python floats (float64 form)."""
    from oracle import replay as orc
    from rltime_amd.history import PrioritizedReplayHistoryBuffer
    from tests.golden.streams import vector_steps, as_reference_samples
    ora = orc.OraclePrioritizedReplay(**tc.long_hist(T), discount_function=orc.make_discount(tc.GAMMA))
    dev = PrioritizedReplayHistoryBuffer(**tc.long_hist(T), gamma=tc.GAMMA)
    spec, step = tc.long_spec(T), 0
    for rnd, (feed_steps, rows, ls) in enumerate(tc.long_rounds(T)):
        for st in vector_steps(spec, feed_steps, start_step=step):
            ora.update(as_reference_samples(spec, st))
            dev.update(as_reference_samples(spec, st))
        step += feed_steps
        ora.update_losses(rows, ls)
        dev.update_losses(rows, ls)
        _check_tree(dev, ora, "T %d round %d" % (T, rnd))
    kinds = {scalar_kind(x) for x in ora.tree.nodes[ora.tree.capacity:] if x != 0}
    assert kinds == {1, 2}
    dev.close()
