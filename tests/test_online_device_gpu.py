"""GPU: DeviceOnlineHistory (history/online_device.py + csrc/actor_critic.hip mirl_online_window) against the host mirror
OnlineHistoryBuffer on the same seeded stream of whole vector steps: the device class gets them as DeviceSamples, the host
class split into per-env dicts (np.float64 rewards, so its arithmetic is float64).  Feed decisions, discard counts, served
order and every batch leaf must agree: returns within 2^-24 |ret| + 2^-40 sum |terms| (one float32 rounding of a float64
sum; the sum of |terms| comes from a second host buffer whose discount function returns the term's magnitude), everything
else bit for bit."""
import numpy as np
import pytest
import torch

from tests import scenario

pytestmark = pytest.mark.gpu

GAMMA, LAM = 0.97, 0.9


def _gae(absolute=False):
    def discount(nstep, reward, po):
        v = po["values"]
        r = po["raw_reward"] if absolute else reward
        term = (GAMMA ** nstep) * (LAM ** (nstep - 1)) * (v + LAM * (r - v))
        return abs(term) if absolute else term
    discount.gamma, discount.lam = GAMMA, LAM
    return discount


def _step(seed, t, E, kind):
    g = np.random.RandomState(7919 * seed + t)
    obs = g.randint(0, 256, size=(E, 2, 4, 4)).astype(np.uint8) if kind == "u8" else g.randn(E, 4).astype(np.float32)
    obs.reshape(E, -1)[:, 0] = np.arange(E)              # the first element names the env: the served order can be read off a batch
    return {"obs": obs, "actions": g.randint(0, 3, size=E).astype(np.int32), "values": g.randn(E).astype(np.float32),
            "logp": (-g.rand(E)).astype(np.float32), "rewards": g.choice([0.0, 1.0, -0.5, 0.25], size=E).astype(np.float32),
            "dones": (g.rand(E) < 0.2).astype(np.uint8)}


def _device_samples(steps, E):
    from rltime_amd.acting.acting_interface import DeviceSamples
    out = DeviceSamples({"x": steps[0]["obs"][0], "layer0_state": {}, "layer1_state": {}}, E, 0)
    for s in steps:
        out.append(frames=torch.from_numpy(s["obs"]).cuda(), actions=torch.from_numpy(s["actions"]).cuda(),
                   policy=torch.from_numpy(np.stack([s["logp"], s["values"]], axis=1)).cuda(),
                   rewards=torch.from_numpy(s["rewards"]).cuda(), dones=torch.from_numpy(s["dones"]).cuda())
    return out


def _dicts(steps, E, absolute=False):
    out = []
    for s in steps:
        for e in range(E):
            r = np.float64(s["rewards"][e])
            out.append({"policy_output": {"actions": s["actions"][e], "values": s["values"][e], "action_log_probs": s["logp"][e],
                                          "raw_reward": r},
                        "next_state": {"x": s["obs"][e], "layer0_state": {}, "layer1_state": {}}, "reward": abs(r) if absolute else r,
                        "done": bool(s["dones"][e]), "info": {}, "env_id": e})
    return out


def _compare(dev, host, mags, tag):
    got = {k: scenario.to_numpy(v) for k, v in scenario.flatten("", dev, {}).items()}
    want = {k: scenario.to_numpy(v) for k, v in scenario.flatten("", host, {}).items()}
    want.pop("policy_outputs.raw_reward")
    assert set(got) == set(want), (sorted(got), sorted(want))
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in scenario.flatten("", dev, {}).values())
    for key in want:
        assert got[key].shape == want[key].shape, (tag, key)
        if key == "returns":
            continue
        assert np.array_equal(got[key].astype(np.float64), want[key].astype(np.float64)), (tag, key)
    assert got["states.x"].dtype == want["states.x"].dtype
    bound = 2.0 ** -24 * np.abs(want["returns"]) + 2.0 ** -40 * mags + 1e-300
    ratio = float(np.max(np.abs(got["returns"].astype(np.float64) - want["returns"]) / bound))
    print("RATIO online.returns %s %.4f" % (tag, ratio))
    assert ratio <= 1.0, tag


@pytest.mark.parametrize("E", [1, 2, 3, 4, 5])
def test_device_history_equals_the_host_history(E):
    from rltime_amd.history.online_device import DeviceOnlineHistory
    from rltime_amd.history.online_history import OnlineHistoryBuffer
    rng = np.random.RandomState(40 + E)
    batches, lost_total, restarts = 0, 0, 0
    for case, (T, n, delay) in enumerate([(3, 3, 5000), (4, 2, 9), (1, 1, 2), (5, 8, 6), (2, 1, 5000)]):
        kind = ("u8", "f32")[(case + E) % 2]
        kw = dict(max_delayed_steps=delay, fixed_target=True, nstep_target=n, nstep_train=T)
        dev = DeviceOnlineHistory(discount_function=_gae(), **kw)
        host = OnlineHistoryBuffer(discount_function=_gae(), **kw)
        mag = OnlineHistoryBuffer(discount_function=_gae(absolute=True), **kw)
        t = 0
        for _ in range(30):
            if rng.rand() < 0.65:
                steps = [_step(100 * E + case, t + i, E, kind) for i in range(int(rng.randint(1, 4)))]
                t += len(steps)
                a, b = dev.update(_device_samples(steps, E)), host.update(_dicts(steps, E))
                mag.update(_dicts(steps, E, absolute=True))
                assert a == b, (E, case)
                lost_total += a["discarded_steps"]
                assert dev.capacity <= max(delay + 1, T + 1)
                continue
            for B in (E - 1, E, E + 1):                  # below, at and above the env count
                if B < 1:
                    continue
                assert dev.needed_feed_count(B, E) == host.needed_feed_count(B, E)
                before = host.last_env
                a, b, m = dev.get_train_data(B), host.get_train_data(B), mag.get_train_data(B)
                assert (a is None) == (b is None)
                if a is None:
                    continue
                batches += 1
                restarts += int(before == 0 and E > 1)
                assert dev.last_env == host.last_env and a["extra_data"] == {}
                assert dev._served == [int(x) for x in np.asarray(b["states"]["x"]).reshape(T, B, -1)[0, :, 0]]      # served order
                _compare(a, b, np.asarray(m["returns"], dtype=np.float64), "E=%d case=%d B=%d" % (E, case, B))
        dev.close()
    assert batches >= 15 and lost_total > 0 and (E == 1 or restarts > 0)


def test_device_history_refuses_what_it_does_not_cover():
    from rltime_amd.history.online_device import DeviceOnlineHistory
    with pytest.raises(ValueError, match="fixed_target"):
        DeviceOnlineHistory(fixed_target=False, nstep_target=2, nstep_train=2, discount_function=_gae())
    with pytest.raises(ValueError, match="gamma"):
        DeviceOnlineHistory(nstep_target=2, nstep_train=2, discount_function=lambda n, r, po: r)
    dev = DeviceOnlineHistory(nstep_target=2, nstep_train=2, discount_function=_gae())
    with pytest.raises(TypeError):
        dev.update([{"env_id": 0}])
    s = _device_samples([_step(1, 0, 2, "f32")], 2)
    s.example_state["layer0_state"] = {"hx": np.zeros(3, np.float32)}
    with pytest.raises(ValueError, match="recurrent"):
        dev.update(s)
