"""Torch float64 restatement of the multi-sample LSTM sequence (csrc/lstm_multi.hip; IQN before the LSTM, merge mode
"inner", reference rltime/models/torch/modules/lstm.py:83-116): everything mirl_lstm_ms_fwd and mirl_lstm_ms_bwd write.
The forward is the loop in the header of lstm_multi.hip; the backward is autograd on float64 leaves, not the kernel's
formulas, so the two are independent.  Shared by the CPU test that ties it to modules.LSTM and the GPU tests that hold
the kernels to it."""
import torch

I = 24          # input width of the test layers


def inputs(T, B, N, H):
    """(parameters, h0, c0, keep, d_out (T, B*N, H)) in float32: unit-scale weights and rows, a reset at t = 0, one in
    mid-sequence, and one that the other rows do not share."""
    g = torch.Generator().manual_seed(1000 * T + 10 * B + N)
    p = dict(x=torch.randn(T * B * N, I, generator=g), w_ih=torch.randn(4 * H, I, generator=g) / I ** 0.5,
             w_hh=torch.randn(4 * H, H, generator=g) / H ** 0.5, bias=torch.randn(4 * H, generator=g) * 0.1)
    h0, c0 = torch.randn(B, H, generator=g) * 0.5, torch.randn(B, H, generator=g)
    keep = (torch.rand(T, B, generator=g) > 0.25).float()
    keep[0, 0] = keep[T // 2, B // 2] = 0.0                 # a reset at t = 0 and one in mid-sequence ...
    keep[0, B - 1] = float(B > 1)                           # ... that the other rows do not share
    up = torch.randn(T, B * N, H, generator=g)
    return p, h0, c0, keep, up


def project(p, T, B, N):
    """gx (T, B, N, 4H) = x W_ih^T + bias in the dtype of p: the part of the op in front of the recurrence."""
    return (p["x"] @ p["w_ih"].t() + p["bias"]).reshape(T, B, N, -1)


def loop(gx, w_hh, h0, c0, keep, cin0=None):
    """The loop of lstm_multi.hip's header in the dtype of gx, differentiable: out (T, B, N, H), hm / cm (T + 1, B, H)
    (masked step inputs, row T the unmasked final state), the activated gates (T, B, N, 4H) in order i, f, g, o, and the
    merged h after every step (the tensors the graph runs through).  cin0 stands in for c0 keep[0] when given."""
    T, B = keep.shape
    h, c = h0.to(gx.dtype), c0.to(gx.dtype)
    out, hm, cm, gates, merged = [], [], [], [], []
    for t in range(T):
        k = keep[t].to(gx.dtype).unsqueeze(1)
        hin, cin = h * k, c * k
        if t == 0 and cin0 is not None:
            cin = cin0
        hm.append(hin)
        cm.append(cin)
        a = gx[t] + (hin @ w_hh.t()).unsqueeze(1)
        ai, af, ag, ao = a.chunk(4, dim=-1)
        gi, gf, gg, go = torch.sigmoid(ai), torch.sigmoid(af), torch.tanh(ag), torch.sigmoid(ao)
        cn = gf * cin.unsqueeze(1) + gi * gg
        hn = go * torch.tanh(cn)
        out.append(hn)
        gates.append(torch.cat([gi, gf, gg, go], dim=-1))
        h, c = hn.mean(1), cn.mean(1)
        merged.append(h)
    return torch.stack(out), torch.stack(hm + [h]), torch.stack(cm + [c]), torch.stack(gates), merged


def loop64(p, h0, c0, keep, N):
    """The reference's inner-mode loop on the float64 leaves p: (out (T, B*N, H), h_T, c_T)."""
    T, B = keep.shape
    out, hm, cm, _, _ = loop(project(p, T, B, N), p["w_hh"], h0.double(), c0.double(), keep)
    return out.reshape(T, B * N, -1), hm[T], cm[T]


def restate(gx, w_hh, h0, c0, keep, d_out):
    """gx (T, B, N, 4H), w_hh (4H, H), h0 / c0 (B, H), keep (T, B), d_out (T, B, N, H) -> dict of float64 tensors:
    out, hm, cm, gates (what mirl_lstm_ms_fwd writes with need_grad), and for the loss sum(out d_out):
      dg     d loss / d pre-activation (T, B, N, 4H), what mirl_lstm_ms_bwd leaves in the gates buffer;
      S      dg summed over n (T, B, 4H);
      dh_ws  as it stands after the sweep: step 0's dh_b = (S[1] W_hh) keep[1], i.e. d loss / d (merged h after
             step 0); zeros when T = 1;
      dc_ws  as it stands after the sweep: d loss / d cin of step 0, before keep[0] is applied."""
    T, B = keep.shape
    gx64 = gx.detach().double().clone().requires_grad_(True)
    cin0 = (c0.double() * keep[0].double().unsqueeze(1)).detach().requires_grad_(True)
    out, hm, cm, gates, merged = loop(gx64, w_hh.detach().double(), h0.double(), c0.double(), keep, cin0)
    if T > 1:
        merged[0].retain_grad()
    (out * d_out.double().reshape(out.shape)).sum().backward()
    dg = gx64.grad
    return dict(out=out.detach(), hm=hm.detach(), cm=cm.detach(), gates=gates.detach(), dg=dg, S=dg.sum(2),
                dh_ws=merged[0].grad if T > 1 else torch.zeros_like(cin0), dc_ws=cin0.grad)


def saturated_inputs(T, B, N, H):
    """(gx, w_hh, h0, c0, keep, d_out) of inputs(T, B, N, H) with about one pre-activation in seven pushed to
    +-(120 .. 180), beyond where the float32 exp of either sign overflows, and one c0 entry in eight set to +-50: every
    gate kind saturates on both sides while most cells stay in the interior."""
    p, h0, c0, keep, up = inputs(T, B, N, H)
    g = torch.Generator().manual_seed(77)
    gx = project(p, T, B, N).clone()
    big = (120.0 + 60.0 * torch.rand(gx.shape, generator=g)) * (1.0 - 2.0 * (torch.rand(gx.shape, generator=g) < 0.5).float())
    gx = torch.where(torch.rand(gx.shape, generator=g) < 0.14, big, gx)
    c0 = c0.clone()
    hit = torch.rand(c0.shape, generator=g) < 0.125
    c0[hit] = 50.0 * (1.0 - 2.0 * (torch.rand(int(hit.sum()), generator=g) < 0.5).float())
    return gx, p["w_hh"], h0, c0, keep, up.reshape(T, B, N, H)
