#!/usr/bin/env python3
"""Times the C51 kernels (csrc/c51.hip k_target_c51 + k_loss_c51) against the same arithmetic as a chain of torch ops
on the GPU (softmax / expectation / argmax / gather / softmax / projection by two index_add_ scatters / clamped
cross-entropy + autograd), at the C51 config's batch (B = 256, T = 1) and at M = 40 960 rows; A = 6 actions, Z = 51
atoms.  One JSON line per (M, path): microseconds per call (median of 50 after 10 warm-up calls) and, for the kernels,
the bytes each moves against the 8 TB/s HBM peak.

    python tools/c51_probe.py"""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rltime_amd.training import qops  # noqa: E402


def torch_chain(lt, ls, sup, r, n, mk, logits, acts, gamma=0.99, vmin=-10.0, vmax=10.0):
    M, A, Z = lt.shape
    with torch.no_grad():
        best = (F.softmax(ls, -1) * sup).sum(2).argmax(1)
        p = F.softmax(lt[torch.arange(M, device=lt.device), best], -1)
        tz = ((r + mk * gamma ** n).unsqueeze(1) * sup).clamp(vmin, vmax)
        b = (tz - vmin) / ((vmax - vmin) / (Z - 1))
        lo, up = b.floor(), b.ceil()
        off = (torch.arange(M, device=lt.device) * Z).unsqueeze(1)
        y = torch.zeros(M * Z, device=lt.device)
        y.index_add_(0, (lo.long() + off).view(-1), (p * (up - b)).view(-1))
        y.index_add_(0, (up.long() + off).view(-1), (p * (b - lo)).view(-1))
        y = y.view(M, Z)
    x = logits.detach().requires_grad_(True)
    q = F.softmax(x[torch.arange(M, device=x.device), acts], -1)
    loss = -(y * q.clamp(1e-5, 1 - 1e-5).log()).sum(1).mean()
    loss.backward()
    return y, x.grad


def fused(lt, ls, sup, r, n, mk, logits, acts):
    y = qops.q_target_c51(lt, ls, sup, r, n, mk, 0.99, -10, 10)
    x = logits.detach().requires_grad_(True)
    loss, _ = qops.c51_loss(x, acts, y)
    loss.backward()
    return y, x.grad


def timed(fn, reps=50, warm=10):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[len(t) // 2]


def one(fn, reps=50):
    """a single launch wrapped in events (the kernel alone)."""
    return timed(fn, reps)


def main():
    A, Z = 6, 51
    for M in (256, 40960):
        g = torch.Generator(device="cuda").manual_seed(M)
        lt, ls, logits = (torch.randn(M, A, Z, device="cuda", generator=g) * 2 for _ in range(3))
        sup = torch.linspace(-10, 10, Z, device="cuda")
        r = torch.randint(-1, 2, (M,), device="cuda", generator=g).float()
        n = torch.ones(M, device="cuda")
        mk = (torch.rand(M, device="cuda", generator=g) > 0.1).float()
        acts = torch.randint(0, A, (M,), device="cuda", generator=g)
        y = qops.q_target_c51(lt, ls, sup, r, n, mk, 0.99, -10, 10)
        t_torch = timed(lambda: torch_chain(lt, ls, sup, r, n, mk, logits, acts))
        t_fused = timed(lambda: fused(lt, ls, sup, r, n, mk, logits, acts))
        t_tgt = one(lambda: qops.q_target_c51(lt, ls, sup, r, n, mk, 0.99, -10, 10))
        t_loss = one(lambda: qops.c51_loss(logits, acts, y))
        bytes_tgt = M * (2 * A * Z * 4 + Z * 4 + 12)
        bytes_loss = M * (Z * 4 * 2 + A * Z * 4 + 8 + 8)
        for rec in (
            {"M": M, "path": "torch op chain (target + cross-entropy loss + backward)", "us": t_torch},
            {"M": M, "path": "fused (qops.q_target_c51 + qops.c51_loss + backward)", "us": t_fused},
            {"M": M, "path": "qops.q_target_c51 alone", "us": t_tgt, "kernel_bytes": bytes_tgt,
             "GBps": bytes_tgt / t_tgt / 1e3, "frac_of_8TBps": bytes_tgt / t_tgt / 1e3 / 8000},
            {"M": M, "path": "qops.c51_loss forward alone (with its wrapper's allocations)", "us": t_loss,
             "kernel_bytes": bytes_loss, "GBps": bytes_loss / t_loss / 1e3, "frac_of_8TBps": bytes_loss / t_loss / 1e3 / 8000},
        ):
            rec.update(A=A, Z=Z)
            print(json.dumps(rec))


if __name__ == "__main__":
    main()
