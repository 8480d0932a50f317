"""Fused LSTM sequence op for the recurrent core (GPU only).

Same recurrence as the reference's LSTMCell time loop with per-step reset
(rltime/models/torch/modules/lstm.py:83-116):

    h_in = h(t-1) * keep(t) ; c_in = c(t-1) * keep(t) ; keep = 1 - initials
    gates = W_ih x(t) + b_ih + W_hh h_in + b_hh       (i, f, g, o)
    c(t) = sig(f) c_in + sig(i) tanh(g) ; h(t) = sig(o) tanh(c(t))

but the input projection of all T steps is ONE GEMM (csrc/gemm3.hip; extra-feature
columns are added by csrc/lstm_extras.hip), and the time loop over it is

  * one persistent launch per sweep (csrc/lstm_seq.hip: W_hh resident in LDS, h
    exchanged between workgroups inside the launch) wherever the shape is covered:
    forward for H in {128, 256, 512} and T >= 2, backward for H = 512 and
    B <= _BWD_PERSISTENT_MAX_B; check_status() reports a sweep that gave up and
    two_sweeps_fit() says whether two forward grids may share the chip;
  * else the per-step path: a forward step is one rocBLAS GEMM accumulated IN PLACE
    onto its slice of the projection + one fused cell kernel (csrc/lstm.hip
    mirl_lstm_cell_fwd), a backward step one cell kernel (mirl_lstm_cell_bwd) + one
    rocBLAS GEMM.

The weight gradients of W_ih and W_hh are one GEMM each over all timesteps after the
backward sweep.
"""
import ctypes as C
import os

import torch

from rltime_amd._lib import lib, check, ptr, stream
from . import gemm3

# (A one-launch step kernel — recurrent GEMM on f32 MFMA with the cell in its epilogue — was built in round 2 and measured no
# faster than GEMM + cell at B = H = 512 (18.8 vs 12.6 + 5.7 us): the gain is in keeping W_hh resident across steps, which the
# persistent kernel below does.  Removed in round 5; at acting batch sizes csrc/actnet.hip k_act_lstm is that idea done right.)

# The persistent sequence kernel (csrc/lstm_seq.hip: one launch per sweep, W_hh resident in
# LDS, h exchanged between workgroups through write-through stores + arrival counters) is
# the default wherever it supports the shape; MIRL_LSTM_PERSISTENT=0 keeps the per-step path.
_PERSISTENT = os.environ.get("MIRL_LSTM_PERSISTENT", "1") != "0"
# The persistent BACKWARD sweep exchanges 32 KB of partial sums per wave and step (write-through);
# measured 13.3 us per step at B = 64 and 17.9 at B = 256, but 28 at B = 512 where the chip-wide
# 64 MB per step saturate the fabric — no better than the cell kernel + rocBLAS GEMM per step
# (20.6 us inside the learner step; profiles/r03_lstm_probe_with_persistent_backward.jsonl).  It is
# therefore the default for small per-GPU batches only (strong scaling: B = 64 per rank at 8 GPUs).
_BWD_PERSISTENT_MAX_B = 128


def check_status(what="a persistent LSTM sweep"):
    """Raise if a persistent sweep has reported failure (a bounded spin gave up on a peer workgroup, or the recurrent state
    became non-finite — the tagged exchange cannot carry inf / nan).  The kernels set a host-visible word; the next
    mirl_lstm_seq_* call also refuses with MIRL_ERR_STATE, but by then the invalid outputs of the failed sweep may have
    reached the optimizer — the trainers call this where the host is already synchronised (log rows, checkpoints) and,
    as a cheap unsynchronised look, before every optimizer step.  Shared-GPU runs that starve the sweep's co-residency
    assumption should set MIRL_LSTM_PERSISTENT=0."""
    st = C.c_int32()
    check(lib.mirl_lstm_seq_status(C.byref(st)), "mirl_lstm_seq_status")
    if st.value:
        raise RuntimeError("%s reported failure (status %d): its outputs are invalid — non-finite recurrent state, or a "
                           "workgroup of the sweep was not resident (another process / stream occupying the GPU: "
                           "MIRL_LSTM_PERSISTENT=0 keeps the per-step kernels)" % (what, st.value))


def persistent_supported(T, B, H):
    return _PERSISTENT and T >= 2 and bool(lib.mirl_lstm_seq_supported(T, B, H))


def two_sweeps_fit(B, H):
    """Can two forward sweeps of this shape run on two streams at once?  The persistent kernel spins on peer workgroups
    and needs its whole grid resident; two grids that do not fit the chip together would starve each other until the
    bounded spin gives up.  True for shapes the per-step path serves (no residency assumption there)."""
    if not (_PERSISTENT and lib.mirl_lstm_seq_supported(2, B, H)):
        return True
    wg, lds, cus, per = C.c_int32(), C.c_int64(), C.c_int32(), C.c_int32()
    check(lib.mirl_lstm_seq_fwd_grid(B, H, C.byref(wg), C.byref(lds), C.byref(cus), C.byref(per)), "mirl_lstm_seq_fwd_grid")
    return 2 * wg.value <= cus.value * per.value


def _sweep_workspace(query, B, H, dev):
    """The workspace of one persistent sweep: `query` (mirl_lstm_seq[_bwd]_workspace_bytes) says how large.  It stays
    allocated until the launch that the caller now enqueues on the current stream has run: record_stream is called here,
    before that launch, which is equivalent (the allocator looks at the recorded streams when the tensor is freed).  Both
    sweeps assert the 256-byte alignment that the entry points require (torch aligns its blocks to 512)."""
    nbytes = C.c_int64()
    check(query(B, H, C.byref(nbytes)))
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    ws.record_stream(torch.cuda.current_stream())
    return ws


def _forward_sweep(gates, w, h0, c0, keep, need_grad):
    """The time loop over `gates` (T, B, 4H) = the input projection (+ biases), in place.
    Returns (out, hm, cm, c_all, h_last, c_last); hm / cm / c_all are None unless need_grad
    (then `gates` holds the activated gates on return)."""
    T, B, G = gates.shape
    H = G // 4
    dev = gates.device
    out = torch.empty((T, B, H), dtype=torch.float32, device=dev)
    st = stream()
    if persistent_supported(T, B, H) and w.data_ptr() % 16 == 0:
        ws = _sweep_workspace(lib.mirl_lstm_seq_workspace_bytes, B, H, dev)
        hm = cm = c_all = h_last = c_last = None
        if need_grad:
            hm = torch.empty((T + 1, B, H), dtype=torch.float32, device=dev)
            cm = torch.empty((T + 1, B, H), dtype=torch.float32, device=dev)
            c_all = torch.empty((T, B, H), dtype=torch.float32, device=dev)
        else:
            h_last = torch.empty((B, H), dtype=torch.float32, device=dev)
            c_last = torch.empty((B, H), dtype=torch.float32, device=dev)
        check(lib.mirl_lstm_seq_fwd(
            T, B, H, ptr(gates), ptr(w), ptr(h0), ptr(c0), ptr(keep), ptr(out), ptr(c_all), ptr(hm), ptr(cm),
            ptr(h_last), ptr(c_last), 1 if need_grad else 0, ptr(ws), st), "mirl_lstm_seq_fwd")
        if need_grad:
            h_last, c_last = hm[T], cm[T]
        return out, hm, cm, c_all, h_last, c_last
    hm = torch.empty((T + 1, B, H), dtype=torch.float32, device=dev)     # masked h inputs; hm[T] = final h
    cm = torch.empty((T + 1, B, H), dtype=torch.float32, device=dev)
    c_all = torch.empty((T, B, H), dtype=torch.float32, device=dev) if need_grad else None
    torch.mul(h0, keep[0].unsqueeze(-1), out=hm[0])
    torch.mul(c0, keep[0].unsqueeze(-1), out=cm[0])
    wt = w.t()
    for t in range(T):
        gates[t].addmm_(hm[t], wt)
        check(lib.mirl_lstm_cell_fwd(
            B, H, ptr(gates[t]), ptr(cm[t]), ptr(keep[t + 1] if t + 1 < T else None),
            ptr(out[t]), ptr(c_all[t] if need_grad else None), ptr(hm[t + 1]), ptr(cm[t + 1]), st),
            "mirl_lstm_cell_fwd")
    return out, hm, cm, c_all, hm[T], cm[T]


def _backward_sweep(gates, c_all, cm, d_out, keep, w):
    """The backward time loop: `gates` (T, B, 4H) activated gates -> d loss / d pre-activation, in place.
    One persistent launch (csrc/lstm_seq.hip k_lstm_seq_bwd) where the shape is covered, else one
    cell kernel + one recurrent GEMM per step."""
    T, B, G = gates.shape
    H = G // 4
    st = stream()
    if _PERSISTENT and T >= 2 and B <= _BWD_PERSISTENT_MAX_B and lib.mirl_lstm_seq_bwd_supported(T, B, H) \
            and w.data_ptr() % 16 == 0:
        ws = _sweep_workspace(lib.mirl_lstm_seq_bwd_workspace_bytes, B, H, gates.device)
        check(lib.mirl_lstm_seq_bwd(T, B, H, ptr(gates), ptr(w), ptr(c_all), ptr(cm), ptr(d_out), ptr(keep), ptr(ws), st),
              "mirl_lstm_seq_bwd")
        return
    dh_rec = torch.empty((B, H), dtype=torch.float32, device=gates.device)
    dc_rec = torch.empty((B, H), dtype=torch.float32, device=gates.device)
    for t in range(T - 1, -1, -1):
        check(lib.mirl_lstm_cell_bwd(
            B, H, ptr(gates[t]), ptr(c_all[t]), ptr(cm[t]), ptr(d_out[t]), ptr(dh_rec), ptr(dc_rec),
            ptr(keep[t + 1] if t + 1 < T else None), 1 if t == T - 1 else 0, st),
            "mirl_lstm_cell_bwd")
        if t > 0:
            torch.mm(gates[t], w, out=dh_rec)


def extras_supported(M, N, X):
    """Does csrc/lstm_extras.hip take an (M, N) gates block with X extra features per row?"""
    return bool(lib.mirl_lstm_extras_supported(M, N, X))


def _row_view(t):
    """(M, N) float32 -> itself when the extras kernels take its rows as stored (16-byte aligned, row stride a multiple
    of 4), else a contiguous copy."""
    t = t.float()
    if t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0:
        return t
    return t.contiguous()


def _compact(extra):
    extra = extra.float()
    return extra if extra.stride(1) == 1 and extra.stride(0) >= extra.shape[1] else extra.contiguous()


def extras_add(src, extra, w_x, out=None):
    """src (M, N) + extra (M, X) @ w_x (N, X)^T  (csrc/lstm_extras.hip: the extra-feature columns of the input
    projection, f32 in a fixed order).  out=None: a fresh buffer, src untouched; out=src: in place.  w_x is the
    strided view W_ih[:, F:] as stored."""
    M, N = src.shape
    X = extra.shape[1]
    extra = _compact(extra)
    w_x = w_x.float()
    if w_x.stride(1) != 1:
        w_x = w_x.contiguous()
    if out is None:
        src = _row_view(src)
        out = torch.empty((M, N), dtype=torch.float32, device=src.device)
    check(lib.mirl_lstm_extras_add(M, N, X, ptr(src), src.stride(0), ptr(extra), extra.stride(0), ptr(w_x), w_x.stride(0),
                                   ptr(out), out.stride(0), stream()), "mirl_lstm_extras_add")
    return out


def extras_wgrad(g, extra):
    """g (M, N)^T @ extra (M, X) -> (N, X): the gradient of W_ih[:, F:], deterministic (no atomics)."""
    g = _row_view(g)
    extra = _compact(extra)
    M, N = g.shape
    X = extra.shape[1]
    need = C.c_int64()
    check(lib.mirl_lstm_extras_wgrad_workspace_bytes(M, N, X, C.byref(need)), "mirl_lstm_extras_wgrad_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=g.device) if need.value else None
    out = torch.empty((N, X), dtype=torch.float32, device=g.device)
    check(lib.mirl_lstm_extras_wgrad(M, N, X, ptr(g), g.stride(0), ptr(extra), extra.stride(0), ptr(out), ptr(ws), need.value,
                                     stream()), "mirl_lstm_extras_wgrad")
    return out


class _ExtrasAdd(torch.autograd.Function):
    """proj + extra @ w_x^T out of place, for a projection formed outside the sequence op (LSTM.project_input)."""

    @staticmethod
    def forward(ctx, proj, extra, w_x):
        ctx.save_for_backward(extra)
        return extras_add(proj, extra, w_x)

    @staticmethod
    def backward(ctx, g):
        extra, = ctx.saved_tensors
        return g, None, (extras_wgrad(g, extra) if ctx.needs_input_grad[2] else None)


def add_extras(proj, extra, w_x):
    return _ExtrasAdd.apply(proj, extra, w_x)


class _LSTMSequence(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_ih, w_hh, bias, h0, c0, keep, track=True, extra=None, w_x=None):
        # x (T*B, I); bias = b_ih + b_hh (4H); keep (T, B).  The input projection of
        # ALL timesteps is one GEMM into `gates`; every step then accumulates the
        # recurrent GEMM onto its slice IN PLACE (no per-step copy of the projection)
        # and the cell kernel turns the pre-activations into activated gates in place.
        T, B = keep.shape
        H = w_hh.shape[1]
        x = x.float()
        w = w_hh.float().contiguous()
        keep = keep.float().contiguous()
        # `track`: decided by the caller from torch.is_grad_enabled() — inside forward() grad mode is
        # always off and ctx.needs_input_grad mirrors requires_grad even in a no_grad pass
        need_grad = track and (any(ctx.needs_input_grad[:4]) or ctx.needs_input_grad[9])
        # with extras: x holds the F feature columns only and w_ih = W_ih[:, :F]; the X extra columns are added to the
        # K = F product in place (csrc/lstm_extras.hip) — the (T*B, F + X) block is never formed
        gates = gemm3.linear_fwd(x, w_ih.float(), bias.float().contiguous())
        if extra is not None:
            extra = _compact(extra)
            extras_add(gates, extra, w_x, out=gates)
        gates = gates.view(T, B, 4 * H)
        out, hm, cm, c_all, h_last, c_last = _forward_sweep(
            gates, w, h0.float().contiguous(), c0.float().contiguous(), keep, need_grad)
        if need_grad:
            ctx.save_for_backward(x, w_ih, gates, c_all, cm, hm, keep, w, extra)
        ctx.mark_non_differentiable(h_last, c_last)
        return out, h_last, c_last

    @staticmethod
    def backward(ctx, d_out, _dh, _dc):
        x, w_ih, gates, c_all, cm, hm, keep, w, extra = ctx.saved_tensors
        T, B, G = gates.shape
        H = G // 4
        d_out = d_out.float().contiguous()
        _backward_sweep(gates, c_all, cm, d_out, keep, w)
        dg = gates.reshape(T * B, G)                      # now d loss / d pre-activation
        d_x = gemm3.grad_input(dg, w_ih.float()) if ctx.needs_input_grad[0] else None
        d_wih = gemm3.grad_weight(dg, x) if ctx.needs_input_grad[1] else None
        d_whh = gemm3.grad_weight(dg, hm[:T].reshape(T * B, H)) if ctx.needs_input_grad[2] else None
        d_b = dg.sum(0) if ctx.needs_input_grad[3] else None
        d_wx = extras_wgrad(dg, extra) if extra is not None and ctx.needs_input_grad[9] else None
        return d_x, d_wih, d_whh, d_b, None, None, None, None, None, d_wx


class _LSTMSequenceFromProjection(torch.autograd.Function):
    """The same recurrence on an input projection computed elsewhere (gx (T, B, 4H) =
    x W_ih^T + b_ih + b_hh, possibly a slice of a larger shared block): gx is left
    untouched (it may have other consumers), so the gates buffer is a copy of it.  With extras (extra (T*B, X),
    w_x = W_ih[:, F:]) gx is the projection of the feature columns alone and the copy is gx + extra w_x^T, made by
    one out-of-place pass (csrc/lstm_extras.hip) that takes the place of the clone."""

    @staticmethod
    def forward(ctx, gx, w_hh, h0, c0, keep, track=True, extra=None, w_x=None):
        T, B, G = gx.shape
        H = G // 4
        w = w_hh.float().contiguous()
        keep = keep.float().contiguous()
        need_grad = track and (ctx.needs_input_grad[0] or ctx.needs_input_grad[1] or ctx.needs_input_grad[7])
        if extra is not None:
            extra = _compact(extra)
            gates = extras_add(gx.reshape(T * B, G), extra, w_x).view(T, B, G)      # a fresh buffer: gx stays as it is
        elif need_grad or not (persistent_supported(T, B, H) and w.data_ptr() % 16 == 0):
            gates = gx.float().clone(memory_format=torch.contiguous_format)
        else:
            gates = gx.float().contiguous()       # the persistent no-grad sweep only READS the projection: no copy
        out, hm, cm, c_all, h_last, c_last = _forward_sweep(
            gates, w, h0.float().contiguous(), c0.float().contiguous(), keep, need_grad)
        if need_grad:
            ctx.save_for_backward(gates, c_all, cm, hm, keep, w, extra)
        ctx.mark_non_differentiable(h_last, c_last)
        return out, h_last, c_last

    @staticmethod
    def backward(ctx, d_out, _dh, _dc):
        gates, c_all, cm, hm, keep, w, extra = ctx.saved_tensors
        T, B, G = gates.shape
        H = G // 4
        d_out = d_out.float().contiguous()
        _backward_sweep(gates, c_all, cm, d_out, keep, w)
        d_whh = gemm3.grad_weight(gates.reshape(T * B, G), hm[:T].reshape(T * B, H)) if ctx.needs_input_grad[1] else None
        d_wx = extras_wgrad(gates.reshape(T * B, G), extra) if extra is not None and ctx.needs_input_grad[7] else None
        return gates, d_whh, None, None, None, None, None, d_wx


def lstm_sequence_from_projection(gx, w_hh, h0, c0, keep, extra=None, w_x=None):
    """gx (T, B, 4H) -> (out (T,B,H), h_T, c_T); with extra (T*B, X) and w_x (4H, X): gx + extra w_x^T."""
    return _LSTMSequenceFromProjection.apply(gx, w_hh, h0, c0, keep, torch.is_grad_enabled(), extra, w_x)


def lstm_sequence(x, w_ih, w_hh, bias, h0, c0, keep, extra=None, w_x=None):
    """x (T*B, I) -> (out (T,B,H), h_T (B,H), c_T (B,H)); keep (T, B) = 1 - initials.  With extra (T*B, X) and
    w_x (4H, X): x and w_ih are the feature columns and the projection is x w_ih^T + extra w_x^T."""
    return _LSTMSequence.apply(x, w_ih, w_hh, bias, h0, c0, keep, torch.is_grad_enabled(), extra, w_x)
