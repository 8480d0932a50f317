"""GPU: mirl_online_append_box (csrc/actor_critic.hip k_online_append with `action_words` 4-byte words per action) against the
NumPy ring restatement of tests/online_append_restate.py with an action ring [cap][E][action_words], the layout
mirl_online_window_box reads; with one word, the ring bytes of mirl_online_append."""
import numpy as np
import pytest
import torch

from tests import online_append_restate as AR

pytestmark = pytest.mark.gpu

E, CAP, OBS_BYTES = 5, 4, 8          # (an 8-byte observation: MountainCar's two float32)


def _append(entry, rings, step, head, k, *words):
    from rltime_amd._lib import lib, check, ptr, stream
    word = torch.tensor([head], dtype=torch.int64, device="cuda")
    d = {name: torch.from_numpy(np.ascontiguousarray(v)).cuda() for name, v in step.items()}
    check(getattr(lib, entry)(E, CAP, ptr(word), k, OBS_BYTES, ptr(d["obs"]), ptr(d["actions"]), ptr(d["rewards"]), ptr(d["dones"]),
                              ptr(d["policy"]), 2, 0, None, None, *[ptr(rings[n]) for n in ("obs", "actions", "rewards", "dones", "policy")],
                              None, None, *words, stream()), entry)
    torch.cuda.synchronize()
    assert int(word) == head


@pytest.mark.parametrize("words", [1, 3, 16])
@pytest.mark.parametrize("head,k", [(0, 0), (CAP - 1, 2), (2 ** 31 + 3, 1)], ids=["first", "wraps", "past-2^31"])
def test_append_box_writes_its_slot_and_nothing_else(words, head, k):
    want = AR.new_rings(CAP, E, OBS_BYTES, 0, canary=True)
    want["actions"] = np.full((CAP, E, words), -77, np.int32)
    step = AR.step_case(17, head + k, E, OBS_BYTES, 0)
    step["actions"] = np.random.RandomState(words + k).randn(E, words).astype(np.float32).view(np.int32)      # float32 components, as bits
    rings, plain = ({name: torch.from_numpy(v).cuda() for name, v in want.items()} for _ in range(2))
    _append("mirl_online_append_box", rings, step, head, k, words)
    assert AR.append(want, head, k, step) == (head + k) % CAP
    for name in ("obs", "actions", "rewards", "dones", "policy"):
        assert np.array_equal(rings[name].cpu().numpy().view(np.uint8), want[name].view(np.uint8)), name
    if words == 1:                   # one word per action: the bytes mirl_online_append leaves
        _append("mirl_online_append", plain, step, head, k)
        assert all(torch.equal(plain[name], rings[name]) for name in plain)


def test_append_box_refuses_a_word_count_outside_1_to_16():
    from rltime_amd._lib import lib
    for words in (0, 17):
        assert lib.mirl_online_append_box(E, CAP, None, 0, OBS_BYTES, *[None] * 5, 2, 0, *[None] * 9, words, None) < 0
