"""CPU: the evaluation counting rule in its prefix-sum form (tests/eval_restate.py, what csrc/acting.hip k_eval_count
computes) against the unmodified reference's own eval_policy on every fixture case (tests/golden/eval_cases.npz, written
by tests/golden/generate_eval.py): episode list, env steps consumed and all ten statistics, bit for bit.  Plus the host
side of the evaluation entry point: eval_policy's parameter list against the reference's, the logger's read-back, and the
refusal of rendering / recording."""
import inspect
import json
import os

import numpy as np
import pytest

from tests.eval_restate import EvalCount, STAT_KEYS, run_stream, stats

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_cases.npz")


@pytest.fixture(scope="module")
def cases():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def case_ids():
    with np.load(GOLDEN) as z:
        return list(range(int(z["num_cases"])))


def test_fixture_holds_the_cases_the_kernel_can_go_wrong_at(cases):
    shapes = [(cases["c%d_rewards" % k].shape[1], int(cases["c%d_n" % k])) for k in range(int(cases["num_cases"]))]
    assert shapes == [(1, 1), (1, 3), (3, 7), (63, 64), (64, 64), (65, 66), (255, 256), (257, 300), (600, 601), (600, 1500)]
    for k in range(len(shapes)):
        r = cases["c%d_rewards" % k]
        assert r.dtype == np.float32 and cases["c%d_dones" % k].dtype == np.uint8
        # multiples of 0.1 in float32: their float64 sums differ from float32 sums, so the accumulation width shows
        assert np.array_equal(r, (np.rint(r.astype(np.float64) * 10).astype(np.float32) * np.float32(0.1)).astype(np.float32))
        assert r.shape[0] >= int(cases["c%d_steps" % k]) + 10


@pytest.mark.parametrize("k", case_ids())
def test_restatement_equals_the_reference(cases, k):
    rewards, dones, N = cases["c%d_rewards" % k], cases["c%d_dones" % k], int(cases["c%d_n" % k])
    ec = run_stream(rewards, dones, N)
    assert ec.finished
    assert int(ec.counters[2]) == int(cases["c%d_steps" % k])
    want = cases["c%d_ep_reward" % k]
    assert ec.ep_reward.dtype == np.float64 and np.array_equal(ec.ep_reward.view(np.uint64), want.view(np.uint64))
    got_r, got_l = stats(list(ec.ep_reward)), stats(list(ec.ep_len))
    for j, s in enumerate(STAT_KEYS):
        assert np.float64(got_r[s]).tobytes() == cases["c%d_reward_stats" % k][j].tobytes(), ("reward", s)
        assert np.float64(got_l[s]).tobytes() == cases["c%d_length_stats" % k][j].tobytes(), ("length", s)


@pytest.mark.parametrize("k", case_ids())
def test_over_run_steps_change_nothing(cases, k):
    rewards, dones, N = cases["c%d_rewards" % k], cases["c%d_dones" % k], int(cases["c%d_n" % k])
    ec = run_stream(rewards, dones, N)
    before = [a.copy() for a in (ec.acc, ec.len, ec.open, ec.counters, ec.ep_reward, ec.ep_len)]
    for t in range(int(ec.counters[2]), rewards.shape[0]):
        ec.step(rewards[t], dones[t])
    for a, b in zip(before, (ec.acc, ec.len, ec.open, ec.counters, ec.ep_reward, ec.ep_len)):
        assert np.array_equal(a, b)


def test_float32_accumulation_would_not_pass(cases):
    """The fixture tells float64 sums of the float32 rewards from float32 sums (what the training tracker keeps)."""
    k = 9
    rewards, dones, N = cases["c%d_rewards" % k], cases["c%d_dones" % k], int(cases["c%d_n" % k])
    acc = np.zeros(rewards.shape[1], np.float32)
    ec, narrow = EvalCount(rewards.shape[1], N), []
    for t in range(int(cases["c%d_steps" % k])):
        acc = acc + rewards[t]
        c = dones[t].astype(bool) & (ec.open != 0)
        narrow.extend(acc[c].astype(np.float64))
        acc[dones[t].astype(bool)] = 0
        ec.step(rewards[t], dones[t])
    assert len(narrow) == N and not np.array_equal(np.array(narrow), cases["c%d_ep_reward" % k])


def test_more_envs_than_episodes_is_refused():
    with pytest.raises(ValueError):
        EvalCount(4, 3)


def test_eval_policy_keeps_the_reference_parameters(cases):
    from rltime_amd.eval import eval_policy
    want = json.loads(str(cases["eval_policy_signature"]))
    got = [[n, None if p.default is inspect.Parameter.empty else p.default]
           for n, p in inspect.signature(eval_policy).parameters.items()]
    assert got[:len(want)] == want
    assert got[len(want):] == [["seed", 0]]


def test_record_and_render_are_refused(tmp_path):
    from rltime_amd.eval import eval_policy
    for kw in ({"record": True}, {"render": True}):
        with pytest.raises(ValueError, match="section 7"):
            eval_policy(str(tmp_path), 1, 1, **kw)
    assert not os.listdir(str(tmp_path))


def test_directory_logger_reads_back_what_it_wrote(tmp_path):
    from rltime_amd.general.loggers import DirectoryLogger, NullLogger
    logger = DirectoryLogger(str(tmp_path / "run"), echo=False)
    config = {"env": "catch", "env_args": {"grid": 6}, "training": {"type": "dqn", "args": {"total_steps": 10}}}
    logger.log_config(config)
    state = {"policy_state": {"w": np.arange(6, dtype=np.float32)}, "train_state": {}}
    logger.save_checkpoint(state, 1234)
    again = DirectoryLogger(str(tmp_path / "run"), echo=False)
    assert again.get_config() == config
    step, data = again.get_checkpoint()
    assert step == 1234 and data.keys() == state.keys()
    assert np.array_equal(data["policy_state"]["w"], state["policy_state"]["w"])
    logger.save_checkpoint(state, 2000)                      # the last checkpoint overwrites (loggers.py:176-184)
    assert again.get_checkpoint()[0] == 2000
    with pytest.raises(RuntimeError):
        NullLogger().get_checkpoint()


def test_eval_record_has_the_reference_keys(cases):
    from rltime_amd.eval import make_record
    ec = run_stream(cases["c2_rewards"], cases["c2_dones"], int(cases["c2_n"]))
    rec = make_record(77, {"episodes": 7, "envs": 3, "steps": int(ec.counters[2]), "reward": stats(list(ec.ep_reward)),
                           "length": stats(list(ec.ep_len))}, 0.5)
    want = json.loads(str(cases["record_keys"]))
    assert sorted(rec) == sorted(want + ["steps", "seconds"])
    line = json.loads(json.dumps(rec, default=str))
    assert line["reward"]["mean"] == float(cases["c2_reward_stats"][0]) and isinstance(line["length"]["max"], int)
