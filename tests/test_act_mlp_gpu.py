"""GPU: csrc/act_mlp.hip — the whole acting network of an MLP Q-learning policy in one launch (mirl_act_mlp_fwd) — through
the C-ABI against the float64 restatement of its layers (tests/act_mlp_restate.py), within the bar
tests/test_actnet_gpu.py::test_head holds the CNN step's head kernels to; its draws against the kernels whose keying it
shares (mirl_cos_embed_rng, mirl_actor_head_rng)."""
import ctypes as C
import functools

import pytest
import torch

from tests import act_mlp_restate as R

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name):
    """The case on the device with its references, computed once: float64 and torch's float32 on the GPU."""
    case = R.Case(name)
    dc = R.DeviceCase(case)
    q64, adv64 = R.reference(case, torch.float64, device="cuda")
    q32, adv32 = R.reference(case, torch.float32, device="cuda")
    return case, dc, (q64, adv64), (q32, adv32)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(None)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_qvalues_and_actions_match_float64(name):
    case, dc, (q64, _), (q32, _) = _case(name)
    actions, q = dc.launch()
    print(name, "err, torch f32 err, scale:", R.check_bar(q, q64, q32))
    clear = R.clear_rows(q64)
    assert int((~clear).sum()) * 8 <= case.E
    assert torch.equal(actions[clear].long(), q64.argmax(1)[clear])
    assert int(actions.min()) >= 0 and int(actions.max()) < case.A


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_a_rerun_repeats_to_the_bit(name):
    case, dc, _, _ = _case(name)
    a1, q1 = dc.launch()
    a2, q2 = dc.launch()
    assert torch.equal(a1, a2) and torch.equal(q1.view(torch.int32), q2.view(torch.int32))


@pytest.mark.parametrize("name", ["shipped-iqn", "no-wave-multiple", "no-leading-layer", "every-limit"])
def test_fractions_drawn_in_the_kernel_are_cos_embed_rngs(name):
    """taus NULL: taus_out equals mirl_cos_embed_rng's draw on the same (seed, step word), and the q-values are the bits
    of the launch that is handed those fractions."""
    from rltime_amd._lib import lib, check
    case, dc, _, _ = _case(name)
    rows, D = case.E * case.N, case.D
    tau_out = torch.full((rows,), -1.0, device="cuda")
    a1, q1 = dc.launch(taus=None, seed=1234, step=11, taus_out=tau_out)
    step = torch.tensor([11], dtype=torch.int64, device="cuda")
    phi = torch.empty((rows, D), device="cuda")
    tau_ref = torch.empty(rows, device="cuda")
    check(lib.mirl_cos_embed_rng(rows, D, 1234, _p(step), _p(dc.freq), _p(phi), _p(tau_ref), _st()), "mirl_cos_embed_rng")
    assert torch.equal(tau_out, tau_ref)
    assert 0.0 <= float(tau_out.min()) and float(tau_out.max()) < 1.0
    a2, q2 = dc.launch(taus=tau_ref, seed=1234, step=11)
    assert torch.equal(q1.view(torch.int32), q2.view(torch.int32)) and torch.equal(a1, a2)
    _, q3 = dc.launch(taus=None, seed=1234, step=12)             # another step word: other fractions
    assert not torch.equal(q1, q3)


def test_epsilon_greedy_draws_are_actor_head_rngs():
    """eps 0.5 on many envs: the explored rows' actions are mirl_actor_head_rng's on the same key, and the explored share
    lies in the band tests/test_actnet_gpu.py::test_head_draws_its_fractions_like_cos_embed_rng uses, scaled to this A:
    a random pick lands on the greedy action 1 / A of the time, so the share is eps (1 - 1 / A) = 0.25 at A = 2; the band
    there, [0.2, 0.65] around 0.4167 at A = 6, is [0.48, 1.56] x the expectation: [0.12, 0.39] here; its lower edge is kept
    as it stands, so the share is held to [0.2, 0.39]."""
    from rltime_amd._lib import lib, check
    E, O, A = 512, 4, 2
    g = torch.Generator().manual_seed(21)
    case = R.Case("shipped-dqn")
    case.E, case.obs = E, torch.randn(E, O, generator=g) * 0.7
    dc = R.DeviceCase(case)
    greedy, q = dc.launch(seed=77, step=11)
    acts, q_e = dc.launch(seed=77, step=11, eps=0.5)
    assert torch.equal(q.view(torch.int32), q_e.view(torch.int32))
    step = torch.tensor([11], dtype=torch.int64, device="cuda")
    eps = torch.tensor(0.5, dtype=torch.float64, device="cuda")
    acts2 = torch.empty(E, dtype=torch.int32, device="cuda")
    q2 = torch.empty(E, A, device="cuda")
    check(lib.mirl_actor_head_rng(E, 1, A, _p(q.contiguous()), A, None, 0, _p(eps), None, 0.0, 77, _p(step), _p(acts2), _p(q2), None, _st()),
          "mirl_actor_head_rng")
    assert torch.equal(greedy, q.argmax(1).int())
    explored = acts != greedy
    share = float(explored.float().mean())
    print("explored share", share)
    assert 0.2 < share < 0.39
    assert torch.equal(acts, acts2)                               # the same selection and the same draws on every row
    assert int(acts.min()) >= 0 and int(acts.max()) < A


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_need_q_0_selects_alike_and_nothing_is_written_past_the_outputs(name):
    """need_q = 0 skips the value stream: qvalues holds the advantage means (within the bar against float64), the actions
    are need_q = 1's on rows clear by 1e-4; canary-filled outputs are written nowhere past E A / E N elements."""
    case, dc, (q64, adv64), (q32, adv32) = _case(name)
    E, A, N = case.E, case.A, case.N
    pad = 64
    qbuf = torch.full((E * A + pad,), -7.0, device="cuda")
    abuf = torch.full((E + pad,), -7, dtype=torch.int32, device="cuda")
    tbuf = torch.full((E * N + pad,), -7.0, device="cuda")
    full_actions, _ = dc.launch()
    actions, _ = dc.launch(need_q=0, actions=abuf, qvalues=qbuf, taus_out=tbuf)
    got = qbuf[:E * A].view(E, A)
    print(name, "err, torch f32 err, scale:", R.check_bar(got, adv64, adv32))
    clear = R.clear_rows(q64) & R.clear_rows(adv64)
    assert int((~clear).sum()) * 8 <= E
    assert torch.equal(abuf[:E][clear], full_actions[clear])
    assert torch.all(qbuf[E * A:] == -7.0) and torch.all(abuf[E:] == -7) and torch.all(tbuf[E * N:] == -7.0)
    if case.D:
        assert torch.equal(tbuf[:E * N], dc.taus)               # handed-in fractions are passed through
    else:
        assert torch.all(tbuf == -7.0)                            # no quantile layer: no fractions
    # the full head under the canaries too
    qbuf.fill_(-7.0)
    dc.launch(need_q=1, actions=abuf, qvalues=qbuf, taus_out=tbuf)
    assert torch.all(qbuf[E * A:] == -7.0) and torch.all(abuf[E:] == -7) and torch.all(tbuf[E * N:] == -7.0)
    R.check_bar(qbuf[:E * A].view(E, A), q64, q32)
