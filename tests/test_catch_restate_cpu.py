"""CPU: the NumPy restatement of Catch (tests/catch_restate.py) on hand-worked cases with the expected arrays written out, the
exact proof that a policy blind to the ball catches with probability 1 / G (the bar of tests/test_catch_learns_gpu.py rests
on it), the uniformity of the restatement's column draw, and the configs / env factory around the new environment."""
import math

import numpy as np
import pytest

from tests import catch_restate as CR

SEED = 1234
B, D = 255, 128                                  # ball, paddle


def _state(ball_col, ball_row, paddle):
    return {"ball_col": np.array([ball_col], np.int64), "ball_row": np.array([ball_row], np.int64),
            "paddle": np.array([paddle], np.int64)}


def _planes(*planes):
    return np.array([planes], dtype=np.uint8)     # (1, P, S, S)


Z4 = [[0, 0, 0, 0]] * 4


def _walk(state, actions, t0, P=4, S=4, G=4, V=4):
    out = []
    for n, a in enumerate(actions):
        state, frames, r, d = CR.catch_step(state, np.array([a]), SEED, t0 + n, P, S, G, V)
        out.append((state, frames, float(r[0]), int(d[0])))
    return out


def test_a_catch_step_by_step():
    """G = 4, one pixel per cell: the ball falls down column 3, the paddle moves right once and waits under it."""
    (s1, f1, r1, d1), (s2, f2, r2, d2), (s3, f3, r3, d3) = _walk(_state(3, 0, [2, 2, 2, 2]), [2, 0, 5], t0=7)
    assert (r1, d1, r2, d2) == (0.0, 0, 0.0, 0)
    assert s1["paddle"].tolist() == [[3, 2, 2, 2]] and s1["ball_row"].tolist() == [1]
    assert np.array_equal(f1, _planes(
        Z4,                                                           # three steps ago: before the episode
        Z4,                                                           # two steps ago: before the episode
        [[0, 0, 0, B], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, D, 0]],     # one step ago: ball row 0, paddle still at 2
        [[0, 0, 0, 0], [0, 0, 0, B], [0, 0, 0, 0], [0, 0, 0, D]]))    # now: ball row 1, paddle at 3
    assert s2["paddle"].tolist() == [[3, 3, 2, 2]]
    assert np.array_equal(f2, _planes(
        Z4,
        [[0, 0, 0, B], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, D, 0]],
        [[0, 0, 0, 0], [0, 0, 0, B], [0, 0, 0, 0], [0, 0, 0, D]],
        [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, B], [0, 0, 0, D]]))
    # third step: ball row 3 = G - 1 over the paddle: +1, done, and the next episode has begun (keyed by t = 9)
    assert (r3, d3) == (1.0, 1)
    col = CR.draw_column(SEED, 9, 0, 4)
    assert s3["ball_col"].tolist() == [col] and s3["ball_row"].tolist() == [0] and s3["paddle"].tolist() == [[2, 2, 2, 2]]
    newest = [[0, 0, 0, 0] for _ in range(4)]
    newest[0][col] = B
    newest[3][2] = D
    assert np.array_equal(f3, _planes(Z4, Z4, Z4, newest))


def test_a_miss():
    (_, _, r1, d1), (_, _, r2, d2), (s3, _, r3, d3) = _walk(_state(0, 0, [2, 2, 2, 2]), [1, 0, 0], t0=1)
    assert (r1, d1, r2, d2) == (0.0, 0, 0.0, 0)
    assert (r3, d3) == (-1.0, 1)                                      # paddle reached column 1, the ball fell down column 0
    assert s3["ball_row"].tolist() == [0]


def test_the_walls_clamp_the_paddle_on_both_sides():
    left = _walk(_state(3, 0, [1, 2, 2, 2]), [1, 1], t0=1)
    assert left[0][0]["paddle"].tolist() == [[0, 1, 2, 2]] and left[1][0]["paddle"].tolist() == [[0, 0, 1, 2]]
    right = _walk(_state(0, 0, [2, 2, 2, 2]), [2, 2], t0=1)
    assert right[0][0]["paddle"].tolist() == [[3, 2, 2, 2]] and right[1][0]["paddle"].tolist() == [[3, 3, 2, 2]]
    assert np.array_equal(right[1][1][0, 3], np.array([[0, 0, 0, 0], [0, 0, 0, 0], [B, 0, 0, 0], [0, 0, 0, D]], np.uint8))


@pytest.mark.parametrize("action", [-1, 3, 4, 9, 0])
def test_out_of_range_actions_leave_the_paddle(action):
    """A = 4: -1, 3 (a valid fourth action), A and A + 5 are all no-ops, like action 0."""
    (s1, f1, r1, d1), = _walk(_state(1, 0, [2, 2, 2, 2]), [action], t0=1)
    assert s1["paddle"].tolist() == [[2, 2, 2, 2]] and (r1, d1) == (0.0, 0)
    assert np.array_equal(f1[0, 3], np.array([[0, 0, 0, 0], [0, B, 0, 0], [0, 0, 0, 0], [0, 0, D, 0]], np.uint8))


def test_reset_shows_one_plane_and_three_zero_planes():
    state, frames, rewards, dones = CR.catch_reset(SEED, 0, 3, 4, 4, 4, 4)
    assert rewards.dtype == np.float32 and not rewards.any() and dones.dtype == np.uint8 and dones.tolist() == [1, 1, 1]
    assert state["ball_row"].tolist() == [0, 0, 0] and state["paddle"].tolist() == [[2, 2, 2, 2]] * 3
    for e in range(3):
        col = CR.draw_column(SEED, 0, e, 4)
        assert state["ball_col"][e] == col
        newest = [[0, 0, 0, 0] for _ in range(4)]
        newest[0][col] = B
        newest[3][2] = D
        assert np.array_equal(frames[e], np.array([Z4, Z4, Z4, newest], np.uint8))      # k = 1..3: zero planes


def test_visible_rows_hide_the_ball_but_not_the_paddle():
    """V = 2 on G = 4: the ball at row 2 is not drawn, the paddle is; the plane one step ago (row 1) still shows it."""
    (_, f1, _, _), (_, f2, _, _) = _walk(_state(0, 0, [2, 2, 2, 2]), [0, 1], t0=1, V=2)
    assert np.array_equal(f2, _planes(
        Z4,
        [[B, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, D, 0]],
        [[0, 0, 0, 0], [B, 0, 0, 0], [0, 0, 0, 0], [0, 0, D, 0]],
        [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, D, 0, 0]]))    # row 2 >= V: paddle only


def test_one_plane_and_four_planes_and_two_pixel_cells():
    st = _state(1, 0, [2, 2, 2, 2])
    (_, f4, _, _), = _walk(st, [2], t0=1, P=4)
    (_, f1, _, _), = _walk(st, [2], t0=1, P=1)
    assert f1.shape == (1, 1, 4, 4) and f4.shape == (1, 4, 4, 4) and np.array_equal(f1[0, 0], f4[0, 3])
    (_, f8, _, _), = _walk(st, [2], t0=1, P=2, S=8)                   # a cell is a 2 x 2 block of pixels
    assert np.array_equal(f8, _planes(
        [[0, 0, B, B, 0, 0, 0, 0], [0, 0, B, B, 0, 0, 0, 0], [0] * 8, [0] * 8, [0] * 8, [0] * 8,
         [0, 0, 0, 0, D, D, 0, 0], [0, 0, 0, 0, D, D, 0, 0]],
        [[0] * 8, [0] * 8, [0, 0, B, B, 0, 0, 0, 0], [0, 0, B, B, 0, 0, 0, 0], [0] * 8, [0] * 8,
         [0, 0, 0, 0, 0, 0, D, D], [0, 0, 0, 0, 0, 0, D, D]]))


def test_records_round_trip():
    st = {"ball_col": np.array([0, 127]), "ball_row": np.array([5, 126]), "paddle": np.array([[1, 2, 3, 4], [127, 0, 126, 5]])}
    rec = CR.records(st)
    assert rec.dtype == np.uint32 and rec.tolist() == [[0, 5, 0x04030201, 0], [127, 126, 0x057E007F, 0]]
    back = CR.from_records(rec)
    assert all(np.array_equal(back[k], st[k]) for k in st)


def test_the_tracking_script_catches_every_ball():
    G, E = 6, 5
    state, _, _, _ = CR.catch_reset(SEED, 0, E, 1, 6, G, G)
    got = []
    for t in range(1, 4 * (G - 1) + 1):
        state, _, r, d = CR.catch_step(state, CR.tracking_action(state), SEED, t, 1, 6, G, G)
        assert d.tolist() == [1 if t % (G - 1) == 0 else 0] * E        # every episode lasts G - 1 steps
        got += r[d == 1].tolist()
    assert got == [1.0] * (4 * E)


# ---- a policy whose actions carry no information about the ball catches with probability exactly 1 / G ---------------------
def _move(dist, action, G):
    out = np.zeros(G)
    for c in range(G):
        out[min(max(c + {1: -1, 2: 1}.get(action, 0), 0), G - 1)] += dist[c]
    return out


def _catch_probability(G, rule):
    """Sum over the ball columns (1 / G each, independent of the actions) of P(the paddle ends on that column), the paddle
    distribution propagated from G // 2 through the episode's G - 1 steps."""
    total = 0.0
    for ball in range(G):
        dist = np.zeros(G)
        dist[G // 2] = 1.0
        for n in range(G - 1):
            dist = rule(dist, n)
        total += dist[ball] / G
    return total


@pytest.mark.parametrize("G", [2, 5, 6, 12])
def test_a_blind_policy_catches_one_ball_in_G(G):
    arbitrary = [2, 2, 1, 0, 7, 2, 1, 1, -1, 2, 2]
    rules = {
        "uniform random": lambda d, n: sum(_move(d, a, G) for a in range(3)) / 3.0,
        "always left": lambda d, n: _move(d, 1, G),
        "a fixed sequence": lambda d, n: _move(d, arbitrary[n], G),
    }
    for name, rule in rules.items():
        assert abs(_catch_probability(G, rule) - 1.0 / G) <= 1e-15, name


def test_the_column_draw_is_uniform():
    G, n = 12, 4096 * 8
    counts = np.zeros(G, np.int64)
    for t in range(4096):
        for e in range(8):
            counts[CR.draw_column(SEED, t, e, G)] += 1
    sigma = math.sqrt(n * (1.0 / G) * (1.0 - 1.0 / G))
    assert counts.sum() == n and np.all(np.abs(counts - n / G) <= 6 * sigma), counts


# ---- configs and the env factory --------------------------------------------------------------------------------------------
def test_the_catch_config_loads_and_validates():
    from rltime_amd.general.config import load_config, validate_config
    cfg = load_config("catch_dqn.json")
    validate_config(cfg)
    assert cfg["env"] == "catch" and tuple(cfg["env_args"]["frame_shape"]) == (4, 84, 84) and cfg["env_args"]["grid"] == 12
    assert cfg["training"]["type"] == "dqn" and cfg["training"]["args"]["history_mode"]["type"] == "replay"


def test_make_vec_env_still_refuses_unknown_names_and_names_catch():
    from rltime_amd.train import make_vec_env
    with pytest.raises(ValueError) as err:
        make_vec_env("Pong-v4", None, 2, "cpu")
    assert "catch" in str(err.value) and "synthetic-atari" in str(err.value)


def test_catch_has_no_cpu_implementation():
    from rltime_amd.train import make_vec_env
    with pytest.raises(ValueError):
        make_vec_env("catch", {"frame_shape": [4, 36, 36], "grid": 6}, 2, "cpu")
