"""Evaluation of a policy as the same one-graph rollout acting uses (reference rltime/eval.py:111-178).

The reference's loop acts with a fixed small epsilon on E envs in parallel and counts the first `episode_count`
episodes that STARTED — not the first that finished, which would favour short episodes (eval.py:59-72).  Here the
K-step rollout graph of acting/fast_step.py (env step + pre-step, input layer, network, head) runs with the replay
ingest replaced by ONE small kernel per vector step, csrc/acting.hip k_eval_count, which applies that counting rule on
the device: running reward (float64) / length per env, the open mask, the two lists.  The host replays the graph until
the kernel's `counted` word reaches N — one 16-byte read per replay, nothing else crosses — then copies the two lists
once and forms the record with the reference's NumPy calls.

The evaluator owns its env, actor, carry and episode tracker; it reads the policy's weights and nothing else of the
training run, and it draws nothing from torch's (or numpy's) global generators: the fused step's draws are Philox
blocks keyed by `seed`, the generic path runs under a forked generator state.  With eps > 0 the random actions come
from the device actor's Philox stream, not the reference's np.random stream: only eps = 0 is comparable run for run."""
import numpy as np
import torch

from rltime_amd._lib import lib, check, ptr, stream
from rltime_amd.exploration.epsilon_greedy import EpsilonGreedyExplorationManager
from .actor import Actor
from .episode_tracker import EpisodeTracker


class EvalSink:
    """The rollout's sink protocol (what a device replay offers fast_step.FastActingStep) with the counting kernel as
    the `ingest` of a vector step.  Nothing is planned on the host and no policy output is kept, so the acting step
    skips the dueling value stream like it does for a replay that stores no q-values.  Rewards arrive raw: the
    evaluator never asks for clipping."""
    _keep_policy = False
    _policy_f32 = 0
    _h = None                                  # no replay handle: the rollout graph is keyed by this object

    def __init__(self, num_envs, episode_count, device):
        E, N = int(num_envs), int(episode_count)
        if E > N:
            raise ValueError("num_envs can't be higher than the requested episode_count (%d > %d)" % (E, N))
        self.E, self.N = E, N
        self.acc = torch.zeros(E, dtype=torch.float64, device=device)
        self.len = torch.zeros(E, dtype=torch.int32, device=device)
        self.open = torch.zeros(E, dtype=torch.uint8, device=device)
        self.counters = torch.zeros(4, dtype=torch.int32, device=device)
        self.ep_reward = torch.zeros(N, dtype=torch.float64, device=device)
        self.ep_len = torch.zeros(N, dtype=torch.int32, device=device)
        self._host_counters = torch.zeros(4, dtype=torch.int32).pin_memory() if torch.cuda.is_available() else None
        self.reset()

    def _launch(self, reset, rewards, dones):
        check(lib.mirl_eval_count(self.E, self.N, reset, ptr(rewards), ptr(dones), ptr(self.acc), ptr(self.len), ptr(self.open),
                                  ptr(self.counters), ptr(self.ep_reward), ptr(self.ep_len), stream()), "mirl_eval_count")

    def reset(self):
        self._launch(1, None, None)

    def count(self, rewards, dones):
        """One vector step: raw float32 rewards [E], uint8 dones [E] (device tensors)."""
        assert rewards.dtype == torch.float32 and dones.dtype == torch.uint8 and rewards.numel() == self.E == dones.numel()
        self._launch(0, rewards, dones)

    def read_counters(self):
        """(started, counted, steps): the one 16-byte read per graph replay."""
        self._host_counters.copy_(self.counters, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return tuple(int(v) for v in self._host_counters[:3])

    # -- the sink protocol ---------------------------------------------------------------------------
    def configure(self, example_state, num_envs, env_base, policy_f32=0):
        assert num_envs == self.E and not policy_f32
        self._h = self                         # configured (a replay sets its library handle here)

    def supports_planned_ingest(self):
        return True

    def plan_ingest(self, iters, num_envs):
        pass                                   # nothing is decided on the host

    def ingest_planned(self, k, obs, actions, rewards, dones, extra=None, state=None, initials=None, policy=None):
        self.count(rewards, dones)

    def update_batch(self, obs, actions, rewards, dones, **kwargs):
        self.count(rewards, dones)


class _QuietTracker(EpisodeTracker):
    """The pre-step kernel keeps its episode rows (they are part of the launch), but nobody reads them back: the
    evaluation's statistics are the counting kernel's."""

    def flush(self):
        self.flushed = self.row


class _ConstantEpsilon(EpsilonGreedyExplorationManager):
    def __init__(self, eps):
        super().__init__(eps_final=eps, exploration_fraction=0.0, eps_start=eps, per_actor_exponent_factor=0)
        self._eps = float(eps)

    def _get_eps(self, progress):
        return self._eps                       # (the schedule's np.random draw for the final-epsilon pick is not made)


class Evaluator:
    def __init__(self, policy, env, episode_count, eps=0.0, seed=0, steps_per_launch=32, fused_mlp=False):
        """fused_mlp (config: acting.extra_args.fused_step): evaluate an MLP policy on float32 vector observations (the device
        CartPole) on the fused MLP step (acting/fast_mlp_step.py); without it such a policy is refused.  A DQN / IQN policy
        acts greedily under the epsilon remap; an actor-critic (A2C / PPO) policy acts by SAMPLING from its Categorical head,
        as the reference's eval does (eval.py:124, actor_predict without force_best), under the same fixed-epsilon remap
        (FastMlpAcStep: words 2 and 3 of the step's Philox block)."""
        if not hasattr(getattr(env, "action_space", None), "n"):
            raise ValueError("Evaluator: the env's action space %r is not Discrete; the evaluation is greedy (arg-max) and the "
                             "reference's has no greedy mode for a Box space either" % (getattr(env, "action_space", None),))
        if not getattr(policy, "is_cuda", lambda: False)():
            raise ValueError("Evaluator: the policy is on the CPU; evaluation runs the device actor (a GPU policy) only")
        if not hasattr(env, "step_device") or torch.device(getattr(env, "device", "cpu")).type != "cuda":
            raise ValueError("Evaluator: the env steps on the host; evaluation needs an env that steps on the device "
                             "('catch', 'synthetic-atari')")
        float_obs = str(getattr(getattr(env, "observation_space", None), "dtype", "")) == "float32"
        if float_obs and not fused_mlp:
            raise ValueError("Evaluator: float32 vector observations (the device CartPole's MLP policies) are not covered: the "
                             "evaluation rides on the fused acting step, which takes CNN policies on uint8 frames only")
        if not 1 <= int(steps_per_launch) <= EpisodeTracker.ROWS:
            raise ValueError("steps_per_launch: 1 .. %d" % EpisodeTracker.ROWS)
        self.policy, self.env = policy, env
        self.E, self.N = int(env.num_envs), int(episode_count)
        self.eps, self.seed, self.K = float(eps), int(seed), int(steps_per_launch)
        self.device = policy.device()
        self.sink = EvalSink(self.E, self.N, self.device)
        ac_mlp = float_obs and hasattr(policy, "actor_head_ac_raw")
        actor = self.actor = Actor(env, device=True, use_graph=True, fused_mlp=fused_mlp, fused_actor_critic=ac_mlp)
        actor._ac_eps_remap = ac_mlp           # (training never remaps an actor-critic policy's actions; the evaluation does)
        if float_obs:
            # the opt-in: the evaluation rides on the fused MLP step or not at all
            from .fast_mlp_step import FastMlpAcStep, FastMlpStep
            why = (FastMlpAcStep if ac_mlp else FastMlpStep).why_not(actor, policy)
            if why is not None:
                raise ValueError("Evaluator: fused_mlp was asked for, but the fused MLP step (acting/fast_mlp_step.py) does not "
                                 "cover this policy / env: %s" % why)
        if self.eps:
            actor._exploration = _ConstantEpsilon(self.eps)
        actor._rng_seed = (self.seed * 0x9E3779B97F4A7C15 + 0xE7A1) & 0x7FFFFFFFFFFFFFFF
        actor._tracker = _QuietTracker(self.E, env.action_space.n, self.device)
        self._started = False
        self.record = None

    def _recurrent(self):
        return [layer for layer in self.policy.model.layers if layer.is_recurrent()]

    def run(self):
        """-> the reference's record (eval.py:164-178 without step / date): episodes, envs, reward and length statistics,
        plus `steps`, the vector steps the counting consumed.  The lists stay in `ep_reward` / `ep_len`."""
        if self._started:
            raise RuntimeError("an Evaluator runs once: its env and carry are consumed")
        self._started = True
        rec = self._recurrent()
        keep = [layer.last_state for layer in rec]           # the eager training actor's carry lives here
        for layer in rec:
            # the evaluation's first input state is all-initial on ITS env count: a carry left by a learner forward has the
            # training batch's rows (restored below)
            layer.last_state = None
        devices = [self.device] if self.device.type == "cuda" else []
        try:
            with torch.random.fork_rng(devices=devices), torch.no_grad():
                # the generic path's draws (torch.rand in the policy / exploration): a stream of the evaluation's own
                torch.default_generator.manual_seed(self.seed)
                if devices:
                    torch.cuda.default_generators[self.device.index if self.device.index is not None
                                                  else torch.cuda.current_device()].manual_seed(self.seed)
                self._run()
        finally:
            for layer, state in zip(rec, keep):
                layer.last_state = state
        return self.record

    def _run(self):
        actor, sink, E = self.actor, self.sink, self.E
        actor.set_actor_policy(self.policy)
        actor.set_sink(sink)
        sink.reset()
        iters = self.K
        self.launches = 0
        while True:
            out = actor.get_samples(iters * E)
            self.launches += 1
            if not getattr(out, "ingested", False):
                # the generic device path (a policy or env the fused step does not cover) hands the steps back: the same
                # kernel, launched per step
                for step in out.vector_steps:
                    sink.count(step["rewards"], step["dones"])
                iters = 1
            started, counted, steps = sink.read_counters()
            if counted >= self.N:
                break
        self.fused = bool(actor._fast)
        self.steps = steps
        self.ep_reward = sink.ep_reward.cpu().numpy()
        self.ep_len = sink.ep_len.cpu().numpy()
        rewards, lengths = list(self.ep_reward), list(self.ep_len)
        self.record = {"episodes": self.N, "envs": E, "steps": steps,
                       **{key: {"mean": np.mean(vals), "min": np.min(vals), "max": np.max(vals), "median": np.median(vals),
                                "std": np.std(vals)} for key, vals in (("reward", rewards), ("length", lengths))}}
