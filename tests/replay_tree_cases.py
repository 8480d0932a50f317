"""Inputs shared by tests/test_replay_tree_cpu.py and tests/test_replay_tree_gpu.py: the PER sampler and tree kernels
(csrc/replay.hip k_per_sample, k_per_sample_global, k_tree_fix, k_recalc_flagged) past the sizes at which they are one
pass over one wave with every heap node in LDS.  No GPU is needed to import this module.

Both files take streams, configurations, loss vectors, uniforms and planted leaves from here, so the CPU file proves
properties of exactly the inputs the GPU file sends.  Expected values are formed on the reference's own scalar objects
(oracle/sumtree.py): a tree is loaded from arrays of (value, kind) and everything above the leaves follows from the plain
operators, NumPy-2 promotion included.
"""
import numpy as np

from oracle.sumtree import SumTree
from tests.golden.streams import StreamSpec, scalar_kind

E = 32
FRAME = (1, 4, 4)
GAMMA = 0.99
LDS_NODES = 2048                  # heap nodes [0, 2048) are read from LDS by both samplers, every child >= 2048 from memory
BATCHES = (1, 63, 64, 65, 1023, 1024, 1025, 3000)
ROUNDS = 3

_T1 = dict(train_frequency=0, nstep_target=1, nstep_train=1, prefix_steps=0, alpha=0.6, beta=0.4)
_SEQ = dict(train_frequency=0, nstep_target=2, prefix_steps=2, alpha=0.9, beta=0.6, max_weight_factor=0.9)

# name -> (stream seed, vector steps fed, tree capacity, sequences whose rows go back as losses, history arguments)
CASES = {
    "t1_1000": (301, 32, 1024, 65, dict(_T1, size=1000)),          # every node staged
    "t1_2000": (302, 63, 2048, 1025, dict(_T1, size=2000)),        # only the leaf level is read from memory
    "t1_3000": (303, 94, 4096, 1025, dict(_T1, size=3000)),
    "t1_5000": (304, 157, 8192, 1025, dict(_T1, size=5000)),       # two inner levels and the leaves from memory
    "t8_3000": (305, 100, 4096, 75, dict(_SEQ, size=3000, nstep_train=8, overlap=7)),    # wave recalc kernel, eviction
    "t4_3000": (306, 100, 4096, 150, dict(_SEQ, size=3000, nstep_train=4, overlap=3)),   # lane recalc kernel
}
GLOBAL_SCALING_CASES = ("t1_5000", "t8_3000")


def spec_of(name):
    return StreamSpec(seed=CASES[name][0], num_envs=E, frame_shape=FRAME, n_actions=4, done_prob=0.03)


def hist_of(name, global_scaling=False):
    return dict(CASES[name][4], global_importance_scaling=bool(global_scaling))


def make_oracle(name, global_scaling=False):
    from oracle import replay as orc
    return orc.OraclePrioritizedReplay(**hist_of(name, global_scaling), discount_function=orc.make_discount(GAMMA))


def feed(name, *buffers):
    from tests.golden.streams import vector_steps, as_reference_samples
    spec = spec_of(name)
    for st in vector_steps(spec, CASES[name][1]):
        for b in buffers:
            b.update(as_reference_samples(spec, st))


def batch_sizes(name, active):
    """Every size of BATCHES the active-sequence count allows, and the case's update size (75 sequences x 8 steps and
    150 x 4 give the 600 loss rows of a sequence case)."""
    return sorted(B for B in set(BATCHES) | {CASES[name][3]} if B <= active)


def uniforms(name, rnd, B):
    return np.random.RandomState(CASES[name][0] * 100003 + rnd * 4099 + B).random_sample(B)


def losses(name, rnd, n):
    """Seeded randn * 0.8, as the stream tests of tests/test_replay_gpu.py feed back."""
    return (np.random.RandomState(CASES[name][0] * 7 + rnd).randn(n) * 0.8).astype(np.float32)


def active_count(ora):
    return len(ora.slot_record) - len(ora.free_slots)


def oracle_slot_table(ora):
    """(slot_env, slot_base) of the oracle, -1 where a slot holds no sequence: what slot_table() reads from the device."""
    se = np.full(ora.n_slots, -1, dtype=np.int64)
    sb = np.full(ora.n_slots, -1, dtype=np.int64)
    for s, head in enumerate(ora.slot_record):
        if head is not None:
            se[s], sb[s] = head["env_id"], head["env_buffer_offset"]
    return se, sb


def sequence_rows(slots, slot_env, slot_base, T):
    """The (env, offset) loss rows of the drawn sequences, one per trained step, duplicates kept (a batch repeats slots)."""
    slots = np.asarray(slots, dtype=np.int64)
    env = np.repeat(np.asarray(slot_env, dtype=np.int64)[slots], T)
    off = (np.asarray(slot_base, dtype=np.int64)[slots][:, None] + np.arange(T)[None, :]).reshape(-1)
    return np.stack([env, off], axis=1)


# ----------------------------------------------------------------------------------------------------------------------
# trees of the reference's scalars from (value, kind) arrays
# ----------------------------------------------------------------------------------------------------------------------
_KIND_TYPES = (float, np.float32, np.float64)          # inverse of tests.golden.streams.scalar_kind


def scalar_of(value, kind):
    return _KIND_TYPES[int(kind)](value)


def load_tree(values, kinds, cls=SumTree):
    """An oracle tree whose leaves are the given scalars and whose inner nodes are re-derived from them, each from its two
    children as segment_tree.py:91-97 does (the result depends on the leaves alone)."""
    cap = len(values)
    tree = cls(cap)
    tree.nodes[cap:] = [scalar_of(v, k) for v, k in zip(values, kinds)]
    for pos in range(cap - 1, 0, -1):
        tree.nodes[pos] = tree.combine(tree.nodes[2 * pos], tree.nodes[2 * pos + 1])
    return tree


def tree_arrays(tree):
    """(values float64, kinds uint8) of all 2 * capacity heap slots; slot 0 is unused."""
    return (np.array([float(x) for x in tree.nodes], dtype=np.float64),
            np.array([scalar_kind(x) for x in tree.nodes], dtype=np.uint8))


def stratified(tree, B, us):
    """prioritized_replay_history.py:235-238 on the tree's scalars: seg = total / B, descend(u * seg + i * seg)."""
    seg = tree.total() / B
    return np.array([tree.descend(float(u) * seg + i * seg) for i, u in enumerate(us)], dtype=np.int64)


def stratum_masses(tree, B, us):
    seg = tree.total() / B
    return [float(u) * seg + i * seg for i, u in enumerate(us)]


def weights(tree, slots, active, beta, min_tree=None):
    """prioritized_replay_history.py:327 per sequence, then :347-354: divided by the batch maximum, or by the weight of
    the smallest priority (p_min form) under global_importance_scaling.  -> (weights, top)."""
    p_sum = tree.total()
    w = np.array([((tree.leaf(int(s)) / p_sum) * active) ** (-beta) for s in slots])
    if min_tree is not None:
        p_min = min_tree.total() / p_sum
        top = (p_min * active) ** (-beta)
    else:
        top = np.max(w)
    w /= top
    return w, top


# ----------------------------------------------------------------------------------------------------------------------
# B. planted ties on both sides of the LDS / memory hand-over (capacity 8192: leaves are heap level 13)
# ----------------------------------------------------------------------------------------------------------------------
PLANT_CASE = "t1_5000"
PLANT_N = 4096                    # leaves [0, 4096) are overwritten; [4096, 5000) keep the fresh Python float 1.0
PLANT_B = 1024
PLANT_TOTAL = 16384               # seg = 16: every stratum mass (u + i) * 16 with u a multiple of 1/16 is an integer
PLANT_PATTERNS = ("weak", "f32", "mixed", "f32_offgrid")
TIE_LEVELS = (9, 10, 11, 12, 13)  # level 10 is the last staged one, 11 the first read from memory, 13 the leaves
OFFGRID = 2.0 ** -30


def planted_ties():
    """[(level, boundary leaf)]: the stratum's mass equals the prefix sum of leaves [0, boundary), which is where the left
    child (level, 2k) ends; the reference goes right on `left == mass`, so the expected slot is `boundary` itself."""
    out = []
    for lvl in TIE_LEVELS:
        width = 1 << (13 - lvl)
        pairs = PLANT_N // (2 * width)
        for k in sorted({int(pairs * (f + 0.04 * (lvl - 9))) for f in (0.03, 0.3, 0.55, 0.8)}):   # apart: one stratum each
            out.append((lvl, (2 * k + 1) * width))
    return out


def planted_leaves(pattern):
    """(values, kinds) of leaves [0, PLANT_N): integers 1..6 that sum to PLANT_TOTAL - 904.  `f32_offgrid`: np.float32
    leaves, except that the left leaf of every level-13 tie is a Python float 2^-30 above its integer.  No float32 is that
    number, so its float32 parent is unchanged, and `leaf > mass` against a float32 mass must be taken in float32."""
    rng = np.random.RandomState(77)
    v = rng.randint(1, 7, size=PLANT_N).astype(np.float64)
    need = int(PLANT_TOTAL - 904 - v.sum())
    pick = np.flatnonzero(v < 6 if need > 0 else v > 1)[:abs(need)]
    assert len(pick) == abs(need)
    v[pick] += np.sign(need)
    i = np.arange(PLANT_N)
    if pattern == "weak":
        k = np.zeros(PLANT_N, dtype=np.uint8)
    elif pattern == "mixed":
        k = ((i + i // 64 + (i >> 4)) % 3).astype(np.uint8)
    else:
        k = np.ones(PLANT_N, dtype=np.uint8)
        if pattern == "f32_offgrid":
            for lvl, b in planted_ties():
                if lvl == 13:
                    v[b - 1] += OFFGRID
                    k[b - 1] = 0
    return v, k


def planted_uniforms():
    """-> (uniforms, [(level, boundary leaf, stratum)]).  Dyadic uniforms <= 15/16; the planted strata land exactly on
    their boundary's prefix sum (the same integers for every kind pattern)."""
    v, _ = planted_leaves("f32")
    prefix = np.concatenate([[0.0], np.cumsum(v)])
    us = np.random.RandomState(78).randint(0, 16, size=PLANT_B) / 16.0
    seg = PLANT_TOTAL // PLANT_B
    ties = []
    for lvl, b in planted_ties():
        P = int(prefix[b])
        us[P // seg] = (P % seg) / float(seg)
        ties.append((lvl, b, P // seg))
    return us, ties


# ----------------------------------------------------------------------------------------------------------------------
# C. more dirty leaves than k_tree_fix has lanes (T = 1: one leaf per distinct transition)
# ----------------------------------------------------------------------------------------------------------------------
FIX_CASE = "t1_5000"
FIX_COUNTS = (1023, 1024, 1025, 2049)


def live_transitions(ora):
    return [(e, ora.env_first_offset[e] + i) for e in sorted(ora.rings) for i in range(len(ora.rings[e]))]


def fix_calls(ora):
    """[(rows (M, 2) int64, losses (M,) float32, distinct transitions)]: four calls naming 1023 ... 2049 distinct live
    transitions, then one whose rows 600 ... 899 repeat rows 0 ... 299 with other losses: the repeats sit in the third and
    fourth 256-row block of the loss kernels, their first occurrences in the first two, and the last row must win."""
    live = np.array(live_transitions(ora), dtype=np.int64)
    out = []
    for j, n in enumerate(FIX_COUNTS):
        rng = np.random.RandomState(900 + j)
        out.append((live[rng.permutation(len(live))[:n]], (rng.randn(n) * 0.8).astype(np.float32), n))
    rng = np.random.RandomState(950)
    rows = live[rng.permutation(len(live))[:600]]
    out.append((np.concatenate([rows, rows[:300]]), (rng.randn(900) * 0.8).astype(np.float32), 600))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# D. the global sampler in one process
# ----------------------------------------------------------------------------------------------------------------------
GLOBAL_CASE = "t8_3000"
GLOBAL_SEED = 0x1D2C3B4A
GLOBAL_BATCHES = (8, 65, 1025, 3000)
GLOBAL_OTHERS = ((2417.3125, 2600.0), (2963.84375, 2750.0))     # fabricated {priority sum, active sequences} of two peers
GLOBAL_DROP = (1, 1025)                                        # (rank, Bg) repeated with rows = half the owned count


def prepare_global(ora, *others):
    """Two update_losses calls on 75 seeded active sequences each (600 rows): the tree then holds fresh np.float64 and
    updated np.float32 leaves side by side, and no sampler call has been made on the shard (its call counter is 0)."""
    T = ora.nstep_train
    for rnd in range(2):
        se, sb = oracle_slot_table(ora)
        rng = np.random.RandomState(700 + rnd)
        picks = rng.permutation(np.flatnonzero(se >= 0))[:75]
        rows = sequence_rows(picks, se, sb, T)
        ls = (rng.randn(len(rows)) * 0.8).astype(np.float32)
        for b in (ora,) + others:
            b.update_losses(rows, ls)


def global_plan():
    """[(call number, rank, Bg)] in call order; the halved-rows repeat is call len(plan) + 1."""
    plan, call = [], 0
    for Bg in GLOBAL_BATCHES:
        for rank in range(3):
            call += 1
            plan.append((call, rank, Bg))
    return plan


def shard_table(rank, own_root, own_active):
    rows = list(GLOBAL_OTHERS)
    rows.insert(rank, (float(own_root), float(own_active)))
    return np.array(rows, dtype=np.float64)


def global_expected(tree, shard, rank, Bg, call, beta):
    """What k_per_sample_global must return for this shard, in stratum order: float64 masses (u_i + i) * (P_g / B_g) on
    the Philox uniforms, C_r the in-order float64 sum of the shards before `rank`, ownership C_r <= mass < C_r + P_r with
    the last rank open above, the local slot by the reference's descent on a np.float64 mass."""
    from tests.test_replay_gpu import _philox_u53
    R = len(shard)
    Pg, Ng, Cr = 0.0, 0.0, 0.0
    for q in range(R):
        if q < rank:
            Cr += float(shard[q, 0])
        Pg += float(shard[q, 0])
        Ng += float(shard[q, 1])
    seg = Pg / float(Bg)
    hi = float("inf") if rank == R - 1 else Cr + float(shard[rank, 0])
    strata, slots, raw, local = [], [], [], []
    for i in range(Bg):
        mass = (_philox_u53(GLOBAL_SEED, call, i) + float(i)) * seg
        if not (mass >= Cr and mass < hi):
            continue
        m = np.float64(mass - Cr)
        s = tree.descend(m)
        strata.append(i); slots.append(s); local.append(float(m))
        raw.append(((np.float64(float(tree.leaf(s))) / np.float64(Pg)) * np.float64(Ng)) ** np.float64(-beta))
    return {"Pg": Pg, "stratum": np.array(strata, dtype=np.int64), "slot": np.array(slots, dtype=np.int64),
            "raw": np.array(raw, dtype=np.float64), "local_mass": np.array(local, dtype=np.float64)}


# ----------------------------------------------------------------------------------------------------------------------
# E. the lane-per-sequence recalc kernel at T > 128 with the summation order visible in the leaf
# ----------------------------------------------------------------------------------------------------------------------
# With the shipped max_weight_factor = 0.9 and alpha < 1 a sum that is one ulp off moves the leaf by a tenth of an ulp, which
# the 1-ulp bar of a leaf (two `pow` implementations) cannot see.  Here the priority is the mean alone, cubed: one ulp of the
# sum becomes three ulps of the leaf, so a pairwise summation that splits anywhere but where NumPy splits is caught.
LONG_T = (136, 200, 264)          # NumPy splits at 64, 96 and 128 (n // 2 rounded down to a multiple of 8: from 68, 100, 132)
LONG_E = 4


def long_spec(T):
    return StreamSpec(seed=400 + T, num_envs=LONG_E, frame_shape=FRAME, n_actions=4, done_prob=0.03)


def long_hist(T):
    return dict(size=20 * T, train_frequency=0, nstep_target=1, nstep_train=T, prefix_steps=0,
                alpha=3.0, beta=0.4, max_weight_factor=0.0)


def long_rounds(T):
    """[(vector steps to feed first, loss rows, losses)].  Round 0: every transition of 3 T steps (all five sequences of
    each env fully updated: the float32 form).  Round 1, after T more steps: offsets [2.5 T, 3.2 T) of each env, so the
    sequences from 2.5 T and 3 T hold updated losses beside fresh Python floats (the float64 form)."""
    rng = np.random.RandomState(500 + T)
    out = []
    for feed_steps, lo, hi in ((3 * T, 0, 3 * T), (T, 5 * T // 2, 16 * T // 5)):
        rows = np.array([(e, o) for e in range(LONG_E) for o in range(lo, hi)], dtype=np.int64)
        out.append((feed_steps, rows, (rng.randn(len(rows)) * 0.8).astype(np.float32)))
    return out


def np_pairwise_sum(a, lo, n, round_split=True):
    """np.add.reduce over a[lo:lo + n] as NumPy's pairwise_sum forms it, in a's own scalar type.  round_split=False leaves
    out the rounding of the split point to a multiple of 8: the planted error this section exists to catch."""
    if n < 8:
        r = a.dtype.type(0)
        for i in range(n):
            r = r + a[lo + i]
        return r
    if n <= 128:
        r = [a[lo + j] for j in range(8)]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] = r[j] + a[lo + i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(i, n):
            res = res + a[lo + i]
        return res
    n2 = n // 2
    if round_split:
        n2 -= n2 % 8
    return np_pairwise_sum(a, lo, n2, round_split) + np_pairwise_sum(a, lo + n2, n - n2, round_split)
