"""CPU: the float64 restatement of the multi-sample LSTM sequence (tests/lstm_multi_restate.py, the reference of the GPU
tests of csrc/lstm_multi.hip) against modules.LSTM's own port of the reference's inner-mode loop, its internal
consistency, and the saturated-input generator: saturated on both sides of every gate kind without being degenerate."""
import numpy as np
import pytest
import torch

from tests import lstm_multi_restate as R


@pytest.mark.parametrize("T,B,N,H", [(3, 5, 3, 32), (2, 3, 2, 48)])
def test_restatement_agrees_with_the_module_loop(T, B, N, H):
    from rltime_amd.models.torch.modules import LSTM
    p, h0, c0, keep, up = R.inputs(T, B, N, H)
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    want = R.loop64(p64, h0, c0, keep, N)
    (want[0] * up.double()).sum().backward()
    m = LSTM((R.I,), H, multi_sample_merge_mode="inner").double()
    m.fused = False
    with torch.no_grad():
        m.lstm_cell.weight_ih.copy_(p["w_ih"])
        m.lstm_cell.weight_hh.copy_(p["w_hh"])
        m.lstm_cell.bias_ih.copy_(p["bias"].double() * 0.25)         # exact parts of the combined bias
        m.lstm_cell.bias_hh.copy_(p["bias"].double() * 0.75)
    x = p["x"].double().requires_grad_(True)
    # only the state stored with timestep 0 is consumed: the other rows must not matter
    hx = torch.cat([h0.double(), torch.full(((T - 1) * B, H), 1e3, dtype=torch.float64)])
    cx = torch.cat([c0.double(), torch.full(((T - 1) * B, H), -1e3, dtype=torch.float64)])
    out = m(x, hx=hx, cx=cx, initials=(1 - keep).double().reshape(-1), timesteps=T)
    (out * up.double().reshape(out.shape)).sum().backward()
    tol = dict(rtol=1e-10, atol=0)
    np.testing.assert_allclose(out.detach().numpy(), want[0].detach().reshape(out.shape).numpy(), **tol)
    np.testing.assert_allclose(m.last_state[0].numpy(), want[1].detach().numpy(), **tol)
    np.testing.assert_allclose(m.last_state[1].numpy(), want[2].detach().numpy(), **tol)
    cell = m.lstm_cell
    for name, got, ref in [("x", x.grad, p64["x"].grad), ("w_ih", cell.weight_ih.grad, p64["w_ih"].grad),
                           ("w_hh", cell.weight_hh.grad, p64["w_hh"].grad), ("bias_ih", cell.bias_ih.grad, p64["bias"].grad),
                           ("bias_hh", cell.bias_hh.grad, p64["bias"].grad)]:
        assert float(ref.abs().max()) > 0
        np.testing.assert_allclose(got.numpy(), ref.numpy(), err_msg=name, **tol)


@pytest.mark.parametrize("T,B,N,H", [(1, 2, 2, 16), (3, 5, 3, 32)])
def test_restatement_backward_quantities_are_what_they_are_called(T, B, N, H):
    """dg, S, dh_ws and dc_ws of restate() against the same gradients taken another way: through the projection's
    leaves, through W_hh (dW_hh = sum_t S[t]^T hm[t]) and through h0 / c0 as leaves."""
    p, h0, c0, keep, up = R.inputs(T, B, N, H)
    p64 = {k: v.double().requires_grad_(True) for k, v in p.items()}
    res = R.restate(R.project(p64, T, B, N), p["w_hh"], h0, c0, keep, up.reshape(T, B, N, H))
    c064 = c0.double().requires_grad_(True)
    out, hm, cm, gates, merged = R.loop(R.project(p64, T, B, N), p64["w_hh"], h0.double(), c064, keep)
    (out * up.double().reshape(out.shape)).sum().backward()
    tol = dict(rtol=1e-10, atol=1e-14)
    for k, v in (("out", out), ("hm", hm), ("cm", cm), ("gates", gates)):
        assert torch.equal(res[k], v.detach()), k
    assert res["dg"].shape == (T, B, N, 4 * H) and res["S"].shape == (T, B, 4 * H)
    np.testing.assert_allclose(res["dg"].sum((0, 1, 2)).numpy(), p64["bias"].grad.numpy(), **tol)
    np.testing.assert_allclose(torch.einsum("tbg,tbh->gh", res["S"], res["hm"][:T]).numpy(), p64["w_hh"].grad.numpy(), **tol)
    np.testing.assert_allclose((res["dc_ws"] * keep[0].double().unsqueeze(1)).numpy(), c064.grad.numpy(), **tol)
    if T == 1:
        assert not bool(res["dh_ws"].any())
    else:
        want = (res["S"][1] @ p["w_hh"].double()) * keep[1].double().unsqueeze(1)
        np.testing.assert_allclose(res["dh_ws"].numpy(), want.numpy(), **tol)
        assert bool(res["dh_ws"].any())
    assert bool(res["dc_ws"][0].any())            # row 0 is reset at t = 0: the gradient BEFORE keep[0] is not zero there


def test_saturated_inputs_saturate_without_being_degenerate():
    T, B, N, H = 3, 5, 3, 32
    gx, w_hh, h0, c0, keep, d_out = R.saturated_inputs(T, B, N, H)
    assert gx.dtype == torch.float32 and bool((c0.abs() == 50).any()) and bool((c0 == 50).any()) and bool((c0 == -50).any())
    res = R.restate(gx, w_hh, h0, c0, keep, d_out)
    a = gx.double() + (res["hm"][:T] @ w_hh.double().t()).unsqueeze(2)
    for kind, part in zip("ifgo", a.chunk(4, dim=-1)):
        assert float(part.max()) > 100 and float(part.min()) < -100, kind
    for k in ("out", "gates"):
        v = res[k]
        pinned = (v.abs() < 1e-6) | ((v.abs() - 1).abs() < 1e-6)
        frac = float(pinned.double().mean())
        print("%s: %.3f of the entries within 1e-6 of 0 or +-1" % (k, frac))
        assert 0 < frac < 0.5, k
    for k, v in res.items():
        assert bool(torch.isfinite(v).all()), k
    assert float(res["dg"].abs().max()) > 0 and float(res["cm"].abs().max()) > 10


def test_shape_gate_and_refusals_are_host_logic():
    """mirl_lstm_ms_supported and the launchers' refusals touch no device: the gate of include/mirl.h, and
    MIRL_ERR_ARG for every shape outside it and for null operands at a shape inside it."""
    from rltime_amd._lib import MIRL_ERR_ARG, lib
    for ok in [(1, 1, 2, 16), (2, 3, 2, 48), (2, 18, 9, 80), (3, 4, 2, 144), (2, 2, 64, 16), (2, 17, 2, 1024), (1, 8, 8, 512)]:
        assert lib.mirl_lstm_ms_supported(*ok) == 1, ok
    bad = [(0, 3, 2, 16), (-1, 3, 2, 16), (2, 0, 2, 16), (2, -1, 2, 16), (2, 3, 1, 16), (2, 3, 0, 16), (2, 3, 65, 16), (2, 3, 2, 8),
           (2, 3, 2, 0), (2, 3, 2, 24), (2, 3, 2, 1040), (2, 3, 2, 1025), (2, 3, 2, 2048)]
    for shape in bad + [(2, 3, 2, 16)]:
        if shape in bad:
            assert lib.mirl_lstm_ms_supported(*shape) == 0, shape
        assert lib.mirl_lstm_ms_fwd(*shape, *([None] * 10), 1, None) == MIRL_ERR_ARG, shape
        assert lib.mirl_lstm_ms_bwd(*shape, *([None] * 8), None) == MIRL_ERR_ARG, shape
