"""GPU: DeviceOnlineHistory with a recurrent policy's pytrees (history/online_device.py + csrc/actor_critic.hip
mirl_online_window_rec) against the host mirror OnlineHistoryBuffer on the seeded stream and the case table of
tests/test_online_device_gpu.py: two recurrent layers of different widths (S = 22), E = 1 ... 5, ring growth, discards, the
`not last_env` restart.  The device class gets the vector steps as the actor packs them (acting/actor.py _pack_state), the host
class the per-env dicts.  Every leaf — hx, cx and initials of both layers included — is bit-exact with the host's dtype and
shape; the returns are within that file's bound."""
import numpy as np
import pytest
import torch

from tests import online_lstm_restate as RL
from tests import scenario
from tests.test_online_device_gpu import _compare, _gae

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("E", [1, 2, 3, 4, 5])
def test_recurrent_device_history_equals_the_host_history(E):
    from rltime_amd.history.online_device import DeviceOnlineHistory
    from rltime_amd.history.online_history import OnlineHistoryBuffer
    rng = np.random.RandomState(40 + E)
    batches, lost_total, restarts, grown, inside = 0, 0, 0, 0, 0
    for case, (T, n, delay) in enumerate([(3, 3, 5000), (4, 2, 9), (1, 1, 2), (5, 8, 6), (2, 1, 5000)]):
        kind = ("u8", "f32")[(case + E) % 2]
        kw = dict(max_delayed_steps=delay, fixed_target=True, nstep_target=n, nstep_train=T)
        dev = DeviceOnlineHistory(discount_function=_gae(), **kw)
        host = OnlineHistoryBuffer(discount_function=_gae(), **kw)
        mag = OnlineHistoryBuffer(discount_function=_gae(absolute=True), **kw)
        t, cap = 0, 0
        for _ in range(30):
            if rng.rand() < 0.65:
                steps = [RL.rec_step(100 * E + case, t + i, E, kind) for i in range(int(rng.randint(1, 4)))]
                t += len(steps)
                a, b = dev.update(RL.rec_device_samples(steps, E)), host.update(RL.rec_dicts(steps, E))
                mag.update(RL.rec_dicts(steps, E, absolute=True))
                assert a == b, (E, case)
                lost_total += a["discarded_steps"]
                assert dev.capacity <= max(delay + 1, T + 1)
                grown += int(cap and dev.capacity > cap)
                cap = dev.capacity
                assert tuple(dev._rings["state"].shape) == (cap, E, 22) and tuple(dev._rings["initials"].shape) == (cap, E)
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
                assert list(a["states"]) == list(b["states"]) and list(a["target_states"]) == list(b["target_states"])
                _compare(a, b, np.asarray(m["returns"], dtype=np.float64), "lstm E=%d case=%d B=%d" % (E, case, B))
                got = {k: scenario.to_numpy(v) for k, v in scenario.flatten("", a, {}).items()}
                want = {k: scenario.to_numpy(v) for k, v in scenario.flatten("", b, {}).items()}
                for side in ("states", "target_states"):
                    for layer, H in (("layer1_state", 3), ("layer2_state", 8)):
                        for name, shape in (("hx", (T, B, H)), ("cx", (T, B, H)), ("initials", (T, B))):
                            key = "%s.%s.%s" % (side, layer, name)
                            assert got[key].dtype == want[key].dtype == np.float32 and got[key].shape == want[key].shape == shape, key
                            assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), key
                inside += int(want["states.layer1_state.initials"][1:].sum())
        dev.close()
    assert batches >= 15 and lost_total > 0 and (E == 1 or restarts > 0) and grown > 0 and inside > 0


def test_recurrent_device_history_refuses_what_does_not_fit_the_layout():
    from rltime_amd.history.online_device import DeviceOnlineHistory

    def fresh():
        return DeviceOnlineHistory(nstep_target=2, nstep_train=2, discount_function=_gae())
    good = RL.rec_device_samples([RL.rec_step(1, 0, 2, "f32")], 2)
    assert fresh().update(good) == {"discarded_steps": 0}
    for drop in ("state", "initials"):                     # a recurrent example_state whose steps lack one of the two blocks
        s = RL.rec_device_samples([RL.rec_step(1, 0, 2, "f32")], 2)
        del s.vector_steps[0][drop]
        with pytest.raises(ValueError, match="recurrent"):
            fresh().update(s)
    s = RL.rec_device_samples([RL.rec_step(1, 0, 2, "f32")], 2)
    s.vector_steps[0]["state"] = s.vector_steps[0]["state"][:, :20].contiguous()      # S disagrees with the layout's 22
    with pytest.raises(ValueError, match="22"):
        fresh().update(s)
    s = RL.rec_device_samples([RL.rec_step(1, 0, 2, "f32")], 2)
    s.vector_steps[0]["initials"] = s.vector_steps[0]["initials"].to(torch.uint8)
    with pytest.raises(ValueError, match="initials"):
        fresh().update(s)
    s = RL.rec_device_samples([RL.rec_step(1, 0, 2, "f32")], 2)
    s.example_state = {"x": s.example_state["x"], "layer0_state": {}}                  # a state block nobody describes
    with pytest.raises(ValueError, match="recurrent"):
        fresh().update(s)
    s = RL.rec_device_samples([RL.rec_step(1, 0, 2, "f32")], 2)
    s.example_state = dict(s.example_state, x=(s.example_state["x"], np.zeros(3, np.float32)))
    with pytest.raises(ValueError, match="extra-feature"):
        fresh().update(s)
