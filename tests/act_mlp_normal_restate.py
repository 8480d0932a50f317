"""The Normal form of the fused MLP acting kernel (csrc/act_mlp.hip k_act_mlp<true, true>) restated: seeded operands laid out as
tests/act_mlp_ac_restate.Case (its DeviceCase launches mirl_act_mlp_ac_fwd on them with A = D), and the in-kernel draws in
float64 NumPy: lane p of env e takes philox_4x32(seed ^ TAG, step, 8 e + p) and forms two normals by Box-Muller."""
import ctypes as C
import math

import numpy as np
import torch

from tests import pointwise_restate as PR

TAG, RNG_SEED, STEPS = 0xB0C5, 0x5EED0B0C5, (5, 2 ** 32 + 7)
# name: (operand seed, E, O, leading widths, HID, D)
SHAPES = {"shipped": (31, 16, 2, [64], 64, 1),                 # mountaincar_continuous_ppo (models/mlp_2x64.json)
          "no-leading-odd-D": (32, 1, 5, [], 20, 3),           # L = 0, a width that is no multiple of 64, the last sine dropped
          "limits": (33, 33, 64, [256, 96], 512, 16),          # every draw lane live, K past one tile, two passes over J
          "moments": (34, 4096, 2, [], 8, 2)}                  # 8192 draws on the smallest trunk


class Case:
    """Linear weights (out, in); wout = [mean_layer.weight; critic.weight], (D + 1, HID).  `A` is D (act_mlp_ac_restate's name)."""

    def __init__(self, name):
        seed, self.E, self.O, self.widths, self.HID, self.A = SHAPES[name]
        self.D, self.NO, self.W = self.A, self.A + 1, self.widths[-1] if self.widths else self.O
        g = torch.Generator().manual_seed(seed)
        rn = lambda *s: torch.randn(*s, generator=g)           # noqa: E731
        self.obs, self.leading, k = rn(self.E, self.O) * 0.7, [], self.O
        for w in self.widths:
            self.leading.append((rn(w, k) / math.sqrt(k), rn(w) * 0.1))
            k = w
        self.wfc, self.bfc = rn(self.HID, self.W) / math.sqrt(self.W), rn(self.HID) * 0.1
        self.wout, self.bout, self.logstd = rn(self.NO, self.HID) / math.sqrt(self.HID), rn(self.NO) * 0.1, rn(self.D) * 0.5

    def ac_shape_args(self):
        return (self.E, self.O, len(self.widths), (C.c_int32 * 2)(*(list(self.widths) + [0, 0])[:2]), self.HID, self.A)


def draws(seed, step, E, D):
    """-> (eps (E, D), the sines an odd D drops (E,)), float64 before the one rounding to float32."""
    w = np.array([[PR.philox_4x32(seed ^ TAG, step, 8 * e + p) for p in range((D + 1) // 2)] for e in range(E)], dtype=np.uint64)
    u1 = ((w[:, :, 0] >> np.uint64(8)).astype(np.float64) + 1.0) / 2.0 ** 24
    u2 = (w[:, :, 1] >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
    r, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
    both = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=2).reshape(E, -1)
    return both[:, :D], both[:, -1]


def launch(dc, logstd, step, seed=RNG_SEED):
    """One mirl_act_mlp_normal_fwd launch on an act_mlp_ac_restate.DeviceCase -> (actions, policy, raw_out, eps_out), NaN-filled before."""
    from rltime_amd._lib import lib, check, ptr, stream
    c, word = dc.case, torch.tensor([step], dtype=torch.int64, device="cuda")
    out = [torch.full(s, float("nan"), device="cuda") for s in ((c.E, c.D), (c.E, 2), (c.E, c.D + 1), (c.E, c.D))]
    check(lib.mirl_act_mlp_normal_fwd(*c.ac_shape_args(), *[ptr(t) for t in (dc.obs, dc.lwT[0], dc.lb[0], dc.lwT[1], dc.lb[1], dc.fcT,
                                      dc.fcb, dc.outT, dc.outb, logstd)], seed, ptr(word), ptr(out[0]), ptr(out[1]), 2, ptr(out[2]),
                                      ptr(out[3]), stream()), "mirl_act_mlp_normal_fwd")
    return out
