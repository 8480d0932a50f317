"""Per-launch device time of the device games' env-step kernels on one GPU (docs/measurement.md, "Flappy on the device"):
k_catch_env_step on (4, 84, 84) frames beside k_flappy_env_step on (4, 84, 84) and (1, 120, 80), at 32 and 256 envs, plain
(`step_into`) and with the actor's pre-step fused in (`step_pre`, H = 512, episode statistics and the action histogram).

`--steps` consecutive steps of one env are captured into ONE HIP graph, which is replayed `--replays` times between two
device events after a warm-up replay: µs per launch with the launch gaps inside the graph and no host in the loop.  The
whole table is taken `--repeats` times in one process.

    python tools/env_step_probe.py [--steps 200] [--replays 20] [--repeats 2]      -> one JSON line per row
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F_PAD, H_PRE = 4224 + 16, 512          # the pre-step writes the carry into the tail of rows this long (flappy_iqn_lstm's)


def pre_args(E, A, actions):
    """mirl_actor_pre's arguments from H on (without the stream), and the tensors they point into."""
    from rltime_amd._lib import ptr
    f = lambda *s: torch.zeros(*s, device="cuda")          # noqa: E731
    i = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")          # noqa: E731
    k = dict(h=f(E, H_PRE), c=f(E, H_PRE), xh=f(E, F_PAD + H_PRE), c_in=f(E, H_PRE), pack=f(E, 2 * H_PRE), ini=f(E), rew=f(E),
             don=torch.zeros(E, dtype=torch.uint8, device="cuda"), epr=f(E), epl=i(E), outr=f(E), outl=i(E), cnt=i(A),
             step=torch.zeros(1, dtype=torch.int64, device="cuda"))
    args = [H_PRE, A, ptr(actions), ptr(k["h"]), ptr(k["c"]), C.c_void_p(k["xh"].data_ptr() + 4 * F_PAD), F_PAD + H_PRE,
            ptr(k["c_in"]), ptr(k["pack"]), ptr(k["ini"]), ptr(k["rew"]), ptr(k["don"]), 1, ptr(k["epr"]), ptr(k["epl"]),
            ptr(k["outr"]), ptr(k["outl"]), ptr(k["cnt"]), ptr(k["step"]), 2 ** 64 - 1]
    return args, k


def measure(make, E, fused, steps, replays):
    from rltime_amd._lib import stream
    env = make(E)
    actions = torch.randint(0, 2, (E,), dtype=torch.int32, device="cuda")
    env.bind_actions(actions)
    obs = env.reset()
    rew, don = torch.empty(E, device="cuda"), torch.empty(E, dtype=torch.uint8, device="cuda")
    pa, keep = pre_args(E, env.action_space.n, actions)

    def body():                            # an even number of steps: the clock parity is back where the capture began
        for _ in range(steps):
            if fused:
                env.step_pre(obs, rew, don, pa + [stream()])
            else:
                env.step_into(obs, rew, don)
    body()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    graph.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(replays):
        graph.replay()
    t1.record()
    torch.cuda.synchronize()
    del keep
    return t0.elapsed_time(t1) * 1000.0 / (steps * replays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    if a.steps % 2:
        ap.error("--steps must be even (the envs' clock pairs alternate)")
    from rltime_amd.acting.catch_env import CatchVecEnv
    from rltime_amd.acting.flappy_env import FlappyVecEnv
    cases = {
        "catch (4,84,84) grid 12": lambda E: CatchVecEnv(E, frame_shape=(4, 84, 84), grid=12, n_actions=3, seed=1),
        "flappy (4,84,84) cell 7": lambda E: FlappyVecEnv(E, frame_shape=(4, 84, 84), cell=7, gap=3, spacing=4, seed=1),
        "flappy (1,120,80) cell 10": lambda E: FlappyVecEnv(E, frame_shape=(1, 120, 80), cell=10, gap=3, spacing=4, seed=1),
    }
    for rep in range(a.repeats):
        for name, make in cases.items():
            for E in (32, 256):
                print(json.dumps({"case": name, "E": E, "repeat": rep,
                                  "step_us": round(measure(make, E, False, a.steps, a.replays), 2),
                                  "step_pre_us": round(measure(make, E, True, a.steps, a.replays), 2)}), flush=True)


if __name__ == "__main__":
    main()
