#!/usr/bin/env python3
"""Golden-vector generator for the distributional DQN (C51) trainer.  Runs ONLY in the
development container, next to tests/golden/generate.py, whose helpers it imports.

Drives the *unmodified* reference DistDQN (training/torch/dist_dqn.py,
policies/torch/dist_dqn.py) on the CPU with seeded inputs, asserts that the CPU
restatement in tests/c51_restate.py reproduces it bit for bit, and writes:

  dist_dqn_cases.npz        calc_target_values and _compute_grads cases
  e2e_dist_dqn_lstm_per.npz the E2E spec (recurrent, dueling, double-Q, burn-in, PER)
                            trained by the reference DistDQN: initial weights, qloss and
                            grad_norm per learner step
  signatures_dist_dqn.json  inspect.signature of both reference classes

    python tests/golden/generate_dist_dqn.py
"""
import copy
import io
import json
import os
import random

import numpy as np
import torch

from generate import HERE, StreamSpec, vector_steps, as_reference_samples, make_trainer, _NullHistory, E2E  # noqa: F401
from tests import c51_restate as c51

from rltime.training.torch.dist_dqn import DistDQN as RefDistDQN  # noqa: E402
from rltime.policies.torch.dist_dqn import DistDQNPolicy as RefDistDQNPolicy  # noqa: E402


class _Stub:
    """predict() returns canned logits; carries the C51 attributes the trainer reads."""

    def __init__(self, logits, Z, vmin, vmax):
        self.logits = logits
        self.num_atoms, self.vmin, self.vmax = Z, vmin, vmax
        self.support = torch.linspace(vmin, vmax, Z)
        self.calls = 0

    def predict(self, x, timesteps):
        self.calls += 1
        return self.logits

    def make_tensor(self, x, non_blocking=False):
        from rltime.models.torch.utils import make_tensor
        return make_tensor(x, "cpu")


# (tag, M, A, Z, double_q, gamma, nstep range)
TARGET_CASES = [
    ("z11", 24, 4, 11, False, 0.99, (1, 4)),
    ("z11_dq", 24, 4, 11, True, 0.97, (1, 4)),
    ("z51", 48, 6, 51, False, 0.99, (1, 6)),
    ("z51_dq", 48, 6, 51, True, 0.99, (1, 6)),
    ("z101_dq", 16, 3, 101, True, 0.9, (1, 3)),
]


def run_target_cases(out, g):
    for tag, M, A, Z, dq, gamma, (n0, n1) in TARGET_CASES:
        lt = torch.randn(M, A, Z, generator=g) * 2
        ls = torch.randn(M, A, Z, generator=g) * 2
        # rewards in {-1, 0, +1} and fractional, a third of the rows terminal
        kind = torch.randint(0, 4, (M,), generator=g)
        ret = torch.where(kind == 3, torch.randn(M, generator=g) * 1.5, (kind - 1).float()).double().numpy()
        nsteps = torch.randint(n0, n1, (M,), generator=g).numpy()
        masks = (torch.arange(M) % 3 != 0).long().numpy()
        t = make_trainer(RefDistDQN, gamma, None, dq)
        t.target_policy = _Stub(lt, Z, -10, 10)
        t.policy = _Stub(ls, Z, -10, 10) if dq else t.target_policy
        y = t.calc_target_values(ret, {}, masks, nsteps, 1)
        f32 = lambda x: torch.from_numpy(np.asarray(x, np.float32))  # noqa: E731
        mine = c51.target(lt, ls if dq else lt, t.policy.support, f32(ret), f32(nsteps), f32(masks), gamma, -10, 10)
        assert torch.equal(y, mine), tag
        for k, v in dict(logits_target=lt, logits_select=ls if dq else lt, returns=ret, nsteps=nsteps, masks=masks,
                         target=y).items():
            out["tg.%s.%s" % (tag, k)] = np.asarray(v)
        out["tg.%s.meta" % tag] = np.array([Z, gamma, -10, 10, int(dq)], np.float64)
        print("target %s: row sums %s" % (tag, np.round(y.sum(1).numpy()[:6], 3)))


def run_loss_cases(out, g):
    T, B, A, Z = 3, 8, 5, 51
    M = T * B
    logits = torch.randn(M, A, Z, generator=g) * 3
    logits[0, :, 0] = 12.0                                # rows where the clamp is active at both ends
    logits[1, :, :] = -8.0
    logits[1, :, 7] = 9.0
    targets = torch.softmax(torch.randn(M, Z, generator=g) * 2, dim=-1)
    targets[2] = 0.0                                      # a dropped-mass target (terminal row, reward 0)
    actions = torch.randint(0, A, (M,), generator=g).numpy()
    actions[0] = actions[1] = 0
    weights = torch.rand(M, generator=g).double().numpy()
    loss_idx = np.stack([np.arange(M) % B, np.arange(M) + 100], 1)
    out.update({"ls.logits": logits.numpy(), "ls.targets": targets.numpy(), "ls.actions": actions,
                "ls.weights": weights, "ls.timesteps": np.array(T)})
    for bm, tm in [("mean", None), ("sum", None), ("mean", "mean"), ("sum", "mean"), ("mean", "sum")]:
        for use_w in (False, True):
            for mode in ("crossentropy", "huber", "mse"):
                tag = "ls.%s.%s.w%d.%s" % (bm, tm, use_w, mode)
                extra = {"loss_indices": loss_idx}
                if use_w:
                    extra["importance_weights"] = weights
                x = logits.clone().requires_grad_(True)
                t = make_trainer(RefDistDQN, 0.99, None, False, 1.0, bm, tm, loss_mode=mode)
                t.history_buffer = _NullHistory()
                t.policy = _Stub(x, Z, -10, 10)
                logged = {}
                real = t.value_log.log

                def tap(key, value, *a, **k):
                    logged[key] = float(value)
                    return real(key, value, *a, **k)
                t.value_log.log = tap
                t._compute_grads({}, targets, {"actions": actions}, extra, T)
                x2 = logits.clone().requires_grad_(True)
                l2, rep2 = c51.loss(x2, actions, targets, torch.from_numpy(weights).float() if use_w else None,
                                    mode, 1.0, T, bm, tm)
                l2.backward()
                assert torch.equal(x.grad, x2.grad), tag
                assert np.array_equal(t.history_buffer.got[1], rep2.detach().numpy()), tag
                assert logged["qloss"] == float(l2.detach()), tag
                out[tag + ".loss"] = np.array(logged["qloss"], np.float32)
                out[tag + ".grad"] = x.grad.numpy()
                out[tag + ".report"] = t.history_buffer.got[1]


def run_e2e_case():
    from rltime.acting.acting_interface import ActingInterface
    import gym
    spec = StreamSpec(**E2E["spec"])

    class ScriptedActor(ActingInterface):
        def __init__(self):
            super().__init__(gym.spaces.Box(0, 255, spec.frame_shape, dtype=np.uint8),
                             gym.spaces.Discrete(spec.n_actions))
            self.t = 0

        def get_env_count(self):
            return spec.num_envs

        def set_actor_policy(self, p):
            pass

        def update_state(self, progress, policy_state=None):
            pass

        def close(self):
            pass

        def get_samples(self, min_samples):
            iters = (max(1, min_samples) + spec.num_envs - 1) // spec.num_envs
            res = []
            for step in vector_steps(spec, iters, start_step=self.t):
                res.extend(as_reference_samples(spec, step, empty_layers=(0, 2)))
            self.t += iters
            return res

    class Quiet:
        def log_result(self, *a, **k):
            pass

        def save_checkpoint(self, *a, **k):
            pass

    cfg = copy.deepcopy(E2E)
    cfg["train"]["vf_scale_epsilon"] = None
    random.seed(cfg["seed"]); np.random.seed(cfg["seed"]); torch.manual_seed(cfg["seed"])
    tr = RefDistDQN(logger=Quiet(), actors=ScriptedActor(), model_config=cfg["model"], policy_args=cfg["policy_args"])
    series = {"qloss": [], "grad_norm": []}
    orig = tr.value_log.log

    def tap(key, value, *a, **k):
        if key in series and k.get("group") == "train":
            series[key].append(float(value))
        return orig(key, value, *a, **k)
    tr.value_log.log = tap
    init = {}
    real_init = tr.init_policies

    def init_and_snapshot():
        real_init()
        for name, pol in (("online", tr.policy), ("target", tr.target_policy)):
            f = io.BytesIO()
            torch.save(pol.state_dict(), f)
            init[name] = np.frombuffer(f.getvalue(), dtype=np.uint8)
    tr.init_policies = init_and_snapshot
    tr.train(**copy.deepcopy(cfg["train"]))
    out = {"config": np.array(json.dumps(cfg)), "qloss": np.array(series["qloss"]),
           "grad_norm": np.array(series["grad_norm"]), "init_online": init["online"], "init_target": init["target"]}
    np.savez_compressed(os.path.join(HERE, "e2e_dist_dqn_lstm_per.npz"), **out)
    print("e2e dist_dqn: %d learner steps, qloss[0..3]=%s" % (len(series["qloss"]), series["qloss"][:4]))


def run_signatures():
    import inspect
    targets = {"policies.DistDQNPolicy": (RefDistDQNPolicy, ["__init__", "_outputs_per_action", "_shape_action_outputs",
                                                            "_actor_predict_postprocess"]),
               "training.DistDQN": (RefDistDQN, ["_train", "create_policy", "calc_target_values", "_compute_grads"])}
    out = {}
    for key, (cls, methods) in targets.items():
        table = {}
        for m in methods:
            params = []
            for name, p in inspect.signature(getattr(cls, m)).parameters.items():
                kind = {p.VAR_POSITIONAL: "*", p.VAR_KEYWORD: "**"}.get(p.kind, "")
                params.append([kind + name, p.default is not p.empty])
            table[m] = params
        out[key] = table
    with open(os.path.join(HERE, "signatures_dist_dqn.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(51)
    cases = {}
    run_target_cases(cases, g)
    run_loss_cases(cases, g)
    np.savez_compressed(os.path.join(HERE, "dist_dqn_cases.npz"), **cases)
    print("dist_dqn cases: %d arrays" % len(cases))
    run_e2e_case()
    run_signatures()
