"""Adam with the global-norm gradient clip in the same two launches (csrc/optim.hip).

reference: rltime/training/torch_trainer.py:177-199 — clip_grad_norm_ followed by torch.optim.Adam.step().  `ClipAdam`
IS a torch.optim.Adam (same state: step / exp_avg / exp_avg_sq per parameter, same state_dict, same param_groups and
lr handling); `step_clipped(clip)` runs norm -> clip -> update as k_adam_sqsum + k_adam_update instead of PyTorch's ~25-60
small launches, and falls back to those (the caller's own clip + `step()`) for anything the kernels do not take.

The step guard (not in the reference): `new_step_guard` allocates the 8 int32 device words, `guard_open`
opens a learner step on them (scan of the priority rows, external status words), and `step_clipped(clip, guard=...)`
takes the guarded update — a step with a veto bit set or a non-finite norm writes nothing."""
import ctypes as C
import importlib

import torch


def _lib():
    return importlib.import_module("rltime_amd._lib")


def _dense_like(a, b):
    """Same element order in memory (the stride of a size-1 dimension says nothing)."""
    return (a.dtype == torch.float32 and a.is_cuda and a.shape == b.shape
            and all(x == y for n, x, y in zip(a.shape, a.stride(), b.stride()) if n > 1))


def _packed(t):
    """numel() elements in numel() consecutive words, in whatever order the strides say."""
    return t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))


VETO_LOSS, VETO_NORM, VETO_STATUS = 1, 2, 4                 # include/mirl.h MIRL_VETO_*
GUARD_WORDS = 8


def new_step_guard(device):
    """The guard's 8 int32 words, zeroed (torch's allocator hands out blocks aligned far beyond the 16 bytes asked for)."""
    g = torch.zeros(GUARD_WORDS, dtype=torch.int32, device=device)
    assert g.data_ptr() % 16 == 0
    return g


def sweep_status_word(device):
    """The persistent LSTM sweeps' status word (csrc/lstm_seq.hip) as a 1-element int32 device tensor over the library's
    own memory, which lives as long as the process.  The first call allocates the word: not inside a graph capture."""
    L = _lib()
    p = C.c_void_p()
    with torch.cuda.device(device):
        L.check(L.lib.mirl_lstm_seq_status_device(C.byref(p)), "mirl_lstm_seq_status_device")
    return _WordView(p.value, device)


class _WordView:
    """A device int32 word that torch does not own: enough of a tensor for guard_open (an address and a device)."""
    def __init__(self, address, device):
        self._address, self.device = int(address), torch.device(device)

    def data_ptr(self):
        return self._address


def guard_open(guard, rows, status=()):
    """mirl_step_guard_open: overwrite word 0 of `guard` with the veto bits of the step about to be applied.  `rows`:
    float32 device tensor of the per-transition errors bound for the replay, or None; `status`: up to 4 int32 device words
    (tensors or sweep_status_word())."""
    L = _lib()
    n = len(status)
    if n > 4:
        raise ValueError("a step guard reads at most 4 status words, got %d" % n)
    if rows is not None:
        rows = rows.detach()
        if not (rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous()):
            raise ValueError("guard_open: rows must be a contiguous float32 device tensor")
    arr = (C.c_void_p * max(n, 1))(*[s.data_ptr() for s in status])
    L.check(L.lib.mirl_step_guard_open(L.ptr(guard), L.ptr(rows), rows.numel() if rows is not None else 0,
                                       arr if n else None, n, L.stream()), "mirl_step_guard_open")


class ClipAdam(torch.optim.Adam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        # capturable: the step counters live on the device (the kernels read and advance them there), so the same object
        # works eagerly and inside a captured graph; lr may be a float or a 0-dim device tensor
        super().__init__(params, lr=lr, betas=betas, eps=eps, capturable=True)
        self._ws = None

    def fused_step_ok(self):
        """One parameter group of dense float32 device tensors whose gradients share their layout."""
        return self.why_not_fused() is None

    def why_not_fused(self):
        if len(self.param_groups) != 1:
            return "more than one parameter group"
        g = self.param_groups[0]
        if g["amsgrad"] or g["weight_decay"] != 0 or g["maximize"] or g.get("differentiable") or g.get("decoupled_weight_decay"):
            return "an Adam variant the kernels do not implement"
        ps = [p for p in g["params"] if p.grad is not None]
        if not ps:
            return "no gradients"
        for i, p in enumerate(ps):
            if not (p.is_cuda and p.dtype == torch.float32 and p.numel() > 0 and _packed(p)):
                return "parameter %d %s %s %s is not a packed float32 device tensor" % (i, tuple(p.shape), p.stride(), p.dtype)
            if not _dense_like(p.grad, p):
                return "gradient %d %s %s does not share its parameter's layout %s" % (i, tuple(p.grad.shape), p.grad.stride(), p.stride())
            st = self.state.get(p)
            if st:       # (a state loaded from another optimizer's checkpoint: the caller then keeps torch's own step)
                if not (_dense_like(st["exp_avg"], p) and _dense_like(st["exp_avg_sq"], p) and torch.is_tensor(st["step"])
                        and st["step"].is_cuda and st["step"].dtype == torch.float32):
                    return "optimizer state %d does not share its parameter's layout / device" % i
        return None

    @torch.no_grad()
    def step_clipped(self, clip, guard=None):
        """-> float32 tensor [norm, norm * coef] (coef = min(clip / (norm + 1e-6), 1); clip None: no scaling).
        The caller checked fused_step_ok().  guard: the int32 device tensor of new_step_guard(), opened for this step by
        guard_open(): the update is then skipped on the device — parameters, gradients, moments and step counters untouched —
        when a veto bit is set or the norm is non-finite, and the guard's counters say so."""
        L = _lib()
        group = self.param_groups[0]
        params, grads, ms, vs, _mx, steps = [], [], [], [], [], []
        self._init_group(group, params, grads, ms, vs, _mx, steps)
        for p, m, v, s in zip(params, ms, vs, steps):
            assert _dense_like(m, p) and _dense_like(v, p) and s.is_cuda and s.dtype == torch.float32      # fused_step_ok()
        n = len(params)
        arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])                   # noqa: E731
        numel = (C.c_int64 * n)(*[p.numel() for p in params])
        dev = params[0].device
        if self._ws is None or self._ws[0] != tuple(numel) or self._ws[1].device != dev:
            need = C.c_int64()
            L.check(L.lib.mirl_adam_clip_workspace_bytes(n, numel, C.byref(need)), "mirl_adam_clip_workspace_bytes")
            self._ws = (tuple(numel), torch.empty(need.value, dtype=torch.uint8, device=dev))
        ws = self._ws[1]
        out = torch.empty(2, dtype=torch.float32, device=dev)
        lr = group["lr"]
        lr_dev = L.ptr(lr) if torch.is_tensor(lr) and lr.is_cuda else None
        b1, b2 = group["betas"]
        args = (n, arr(params), arr(grads), arr(ms), arr(vs), arr(steps), numel,
                float(lr) if lr_dev is None else 0.0, lr_dev, float(b1), float(b2), float(group["eps"]),
                float(clip) if clip is not None else 0.0, L.ptr(ws), ws.numel(), L.ptr(out))
        if guard is None:
            L.check(L.lib.mirl_adam_clip_step(*args, L.stream()), "mirl_adam_clip_step")
        else:
            L.check(L.lib.mirl_adam_clip_step_guarded(*args, L.ptr(guard), L.stream()), "mirl_adam_clip_step_guarded")
        # the kernels wrote through raw pointers: move the version counters like the in-place tensor ops they replace
        # (the caches of derived weights — joint / permuted / packed copies, models/torch/gemm3.py — are keyed by them)
        torch.autograd.graph.increment_version(params + grads + ms + vs + steps)
        return out
