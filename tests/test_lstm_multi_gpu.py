"""GPU: the multi-sample LSTM sequence (IQN before the LSTM, merge mode "inner"; csrc/lstm_multi.hip) against the
reference's time loop (modules/lstm.py:83-116) written in plain torch float64 on the CPU, the routing of LSTM.forward,
and configs/catch_iqn_lstm_pre.json end to end."""
import copy

import numpy as np
import pytest
import torch

from tests.lstm_multi_restate import I, inputs as _inputs, loop64 as _loop64

pytestmark = pytest.mark.gpu

OUT_TOL = dict(rtol=1e-4, atol=2e-5)
GRAD_TOL = dict(rtol=1e-3, atol=2e-5)
# one step / one sequence (idle waves, idle rows); odd N, ragged row tile; across a row tile at the recommended N = 8;
# the default N = 32; the full K loops with S staged in chunks
SHAPES = [(1, 1, 2, 16), (3, 5, 3, 32), (4, 17, 8, 64), (2, 33, 32, 128), (3, 16, 8, 512)]


@pytest.mark.parametrize("T,B,N,H", SHAPES)
def test_op_against_float64(T, B, N, H):
    from rltime_amd._lib import lib, check, ptr, stream
    from rltime_amd.models.torch import lstm_seq
    p, h0, c0, keep, up = _inputs(T, B, N, H)
    assert lstm_seq.multi_supported(T, B, N, H)
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    want = _loop64(p64, h0, c0, keep, N)
    (want[0] * up.double()).sum().backward()
    dev = {k: v.cuda().requires_grad_(True) for k, v in p.items()}
    got = lstm_seq.lstm_sequence_multi(dev["x"], dev["w_ih"], dev["w_hh"], dev["bias"], h0.cuda(), c0.cuda(), keep.cuda(), N)
    (got[0] * up.cuda()).sum().backward()
    for a, b in zip(got, want):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), **OUT_TOL)
    for k in p:
        scale = float(p64[k].grad.abs().max()) + 1e-6
        np.testing.assert_allclose(dev[k].grad.cpu().numpy() / scale, p64[k].grad.numpy() / scale, err_msg=k, **GRAD_TOL)
    # the entry point itself: need_grad = 0 only reads gx and gives the bits of the need_grad = 1 pass
    gx0 = (p["x"] @ p["w_ih"].t() + p["bias"]).cuda()
    w, h0d, c0d, keepd = dev["w_hh"].detach(), h0.cuda(), c0.cuda(), keep.cuda()
    res = []
    for need_grad in (0, 1):
        gx, out = gx0.clone(), torch.empty(T, B, N, H, device="cuda")
        hm, cm = torch.empty(T + 1, B, H, device="cuda"), torch.empty(T + 1, B, H, device="cuda")
        check(lib.mirl_lstm_ms_fwd(T, B, N, H, ptr(gx), ptr(w), ptr(h0d), ptr(c0d), ptr(keepd), ptr(out), ptr(hm), ptr(cm),
                                   None, None, need_grad, stream()), "mirl_lstm_ms_fwd")
        res.append((gx, out, hm, cm))
    assert torch.equal(res[0][0], gx0) and not torch.equal(res[1][0], gx0)
    assert all(torch.equal(a, b) for a, b in zip(res[0][1:], res[1][1:]))
    np.testing.assert_allclose(res[0][1].reshape(T, B * N, H).cpu().numpy(), want[0].detach().numpy(), **OUT_TOL)


@pytest.mark.parametrize("mode", ["inner", "outer"])
def test_module_routes_inner_mode_to_the_op(mode, monkeypatch):
    from rltime_amd.models.torch import lstm_seq
    from rltime_amd.models.torch.modules import LSTM
    T, B, N, H = 3, 5, 3, 32
    calls = []
    real = lstm_seq.lib.mirl_lstm_ms_fwd
    monkeypatch.setattr(lstm_seq.lib, "mirl_lstm_ms_fwd", lambda *a: calls.append(a[:4]) or real(*a))
    torch.manual_seed(5)
    a = LSTM((I,), H, multi_sample_merge_mode=mode).cuda()
    b = copy.deepcopy(a)
    b.fused = False
    g = torch.Generator().manual_seed(2)
    x = torch.randn(T * B * N, I, generator=g).cuda()
    hx, cx = torch.randn(T * B, H, generator=g).cuda(), torch.randn(T * B, H, generator=g).cuda()
    initials = (torch.rand(T * B, generator=g) < 0.3).float().cuda()
    up = torch.randn(T * B * N, H, generator=g).cuda()
    res = []
    for m in (a, b):
        xi = x.clone().requires_grad_(True)
        out = m(xi, hx=hx, cx=cx, initials=initials, timesteps=T)
        (out * up).sum().backward()
        res.append([out.detach(), m.last_state[0], m.last_state[1], xi.grad] + [q.grad for q in m.parameters()])
    if mode == "outer":
        assert not calls and all(torch.equal(u, v) for u, v in zip(*res))
        return
    assert calls == [(T, B, N, H)]
    for i, (u, v) in enumerate(zip(*res)):
        scale = 1.0 if i < 3 else float(v.abs().max()) + 1e-6
        np.testing.assert_allclose(u.cpu().numpy() / scale, v.cpu().numpy() / scale, err_msg=str(i), **(OUT_TOL if i < 3 else GRAD_TOL))


def test_shipped_config_trains_through_the_op(monkeypatch):
    """configs/catch_iqn_lstm_pre.json cut down: a handful of learner steps, finite losses, and both the learner's
    sequences and the actor's T = 1 steps reach mirl_lstm_ms_fwd."""
    import random
    from rltime_amd.general.config import load_config
    from rltime_amd.general.loggers import NullLogger
    from rltime_amd.models.torch import lstm_seq
    from rltime_amd.train import train
    steps = []
    real = lstm_seq.lib.mirl_lstm_ms_fwd
    monkeypatch.setattr(lstm_seq.lib, "mirl_lstm_ms_fwd", lambda *a: steps.append(a[0]) or real(*a))
    random.seed(0); np.random.seed(0); torch.manual_seed(0)      # noqa: E702
    cfg = load_config("catch_iqn_lstm_pre.json")
    assert cfg["policy_args"]["num_sampling_quantiles"] == 8 and cfg["policy_args"]["injection_layer"] == 1
    cfg["acting"]["actor_envs"] = 8
    cfg["training"]["args"].update(mbatch_size=4, nstep_train=8, burn_in_timesteps=0, total_steps=360, warmup_steps=200,
                                   log_freq=180, target_update_freq=100)
    cfg["training"]["args"]["history_mode"]["args"].update(size=400, train_frequency=4)
    logger = NullLogger()
    trainer = train(copy.deepcopy(cfg), logger)
    assert not trainer.actors._fast
    losses = [row["train"]["qloss"] for name, _, row in logger.rows if name == "train" and "qloss" in row.get("train", {})]
    assert losses and all(np.isfinite(float(v)) for v in losses), losses
    assert all(bool(torch.isfinite(q).all()) for q in trainer.policy.parameters())
    assert 1 in steps and max(steps) > 1
