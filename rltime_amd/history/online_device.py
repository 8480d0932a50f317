"""On-policy ("online") history on the device, for A2C / PPO with the device-resident actor (reference
rltime/history/online_history.py:4-120 over history.py:71-286; the host mirror is history/online_history.py).

The actor hands whole vector steps (acting_interface.DeviceSamples): `update` appends them to device rings, one slot per
vector step, with no host copy and no synchronisation.  Everything the reference decides on the host is data-independent
— which envs are served round-robin, the `not last_env` quirk, how many transitions each env has pending, the
max_delayed_steps discards, the feed decision, an env's very first transition starting from its own next_state — and
stays on the host as plain Python (`OnlinePlan`, no torch).  `get_train_data` uploads the plan of the served sequences
(env, first ring slot) and one launch of csrc/actor_critic.hip (mirl_online_window) writes the (T, B) batch: lambda-returns
in float64, step counts, masks, the gathered policy outputs and both observation blocks.

A recurrent policy's next_state also carries each recurrent layer's hx, cx and the `initials` flag.  The vector steps hand
them over packed (`state` [E, S], `initials` [E]: acting/actor.py _pack_state), two more rings keep them, and the same
launch (mirl_online_window_rec) moves them from exactly the ring rows the observations come from; the stored pytree is
described by the replay's _Layout, which is where the field order is stated.

The history is also a SINK of the fused acting step (acting/fast_step.py), with the protocol that step speaks to the device
replay: `configure`, `update_batch` (one vector step from the step's static buffers) and `plan_ingest` + `ingest_planned`
(a whole rollout captured into one HIP graph).  Both make ONE launch per vector step (mirl_online_append) whose ring slot is
(head word + k) mod capacity with the head word on the device, so a captured rollout lands in the right slots at every ring
position; the host bookkeeping (`OnlinePlan.feed`, growing the rings) runs before the launch.
"""
import itertools

import numpy as np
import torch

from .replay_history import _Layout


class OnlinePlan:
    """The host bookkeeping of OnlineHistoryBuffer for envs that are fed in whole vector steps.  Vector step number s
    (counted from 0) lives in ring slot s % capacity; env e's pending transitions are the last pending[e] vector steps."""

    def __init__(self, nstep_train, max_delayed_steps):
        self.nstep_train, self.max_delayed_steps = nstep_train, max_delayed_steps
        self.pending = {}          # env id -> transitions not handed out yet
        self.first_step = {}       # env id -> the vector step of its first ever transition
        self.head = 0              # vector steps fed so far
        self.last_env = None

    def feed(self, env_ids):
        """One vector step -> transitions discarded (online_history.py:61-73)."""
        discarded = 0
        for e in env_ids:
            if e not in self.pending:
                self.pending[e], self.first_step[e] = 0, self.head
            self.pending[e] += 1
            if self.pending[e] > self.max_delayed_steps:
                self.pending[e] -= 1
                discarded += 1
        self.head += 1
        return discarded

    def live_steps(self):
        """Vector steps the rings must hold: the longest pending run and the step before it (its first state)."""
        return max(self.pending.values(), default=0) + 1

    def sequences_ready(self):
        return sum(n // self.nstep_train for n in self.pending.values())

    def steps_until_ready(self, mbatch_size, env_ids):
        """The smallest number n >= 1 of whole vector steps of `env_ids` after which sequences_ready() >= mbatch_size, or
        None when no number of steps gets there.  n feeds leave env e with min(pending[e] + n, max_delayed_steps)
        transitions, so the count of ready sequences is a non-decreasing step function of n, constant from
        n = max_delayed_steps on: bisection over [1, max_delayed_steps]."""
        T, D = self.nstep_train, self.max_delayed_steps
        have = {e: self.pending.get(e, 0) for e in set(self.pending) | set(env_ids)}
        fed = set(env_ids)

        def ready(n):
            return sum(min(p + (n if e in fed else 0), max(D, p)) // T for e, p in have.items())
        if D < 1 or ready(D) < mbatch_size:
            return None
        lo, hi = 1, D
        while lo < hi:
            mid = (lo + hi) // 2
            if ready(mid) >= mbatch_size:
                hi = mid
            else:
                lo = mid + 1
        return lo

    def serve(self, mbatch_size):
        """online_history.py:81-120 -> [(env id, vector step of the sequence's first transition, 1 if that is the env's
        first ever transition)] in the served order, or None = feed more."""
        T = self.nstep_train
        if self.sequences_ready() < mbatch_size:
            return None
        ids = sorted(self.pending)
        # (`not last_env`, online_history.py:101-103: env id 0 restarts the walk like "none served yet")
        at = 0 if not self.last_env else (ids.index(self.last_env) + 1) % len(ids)
        out = []
        while len(out) < mbatch_size:
            env = ids[at]
            if self.pending[env] >= T:
                start = self.head - self.pending[env]
                out.append((env, start, int(start == self.first_step[env])))
                self.pending[env] -= T
                self.last_env = env
            at = (at + 1) % len(ids)
        return out


class _RingHandle:
    """What FastActingStep keys its captured rollouts with: `value` changes whenever the rings are reallocated, so a graph
    that holds freed ring pointers is never replayed."""
    _next = itertools.count(1)

    def __init__(self):
        self.renew()

    def renew(self):
        self.value = next(_RingHandle._next)


class DeviceOnlineHistory:
    _keep_policy = True            # the [log-probability | value] pair of every transition is stored

    def __init__(self, max_delayed_steps=5000, fixed_target=True, **kwargs):
        """online_history.py:21-47; **kwargs are History's (nstep_target, nstep_train, prefix_steps=0,
        discount_function=None, state_store=None).  The discount function must be A2C's (training/a2c.py): its `.gamma`
        and `.lam` are what the kernel evaluates."""
        self._base_init(**kwargs)
        if not fixed_target:
            raise ValueError("DeviceOnlineHistory: fixed_target=False is not supported on the device path: its targets "
                             "look past the training window")
        if self.prefix_steps:
            raise ValueError("Online history does not support prefix/burnin steps")
        fn = self.discount_function
        if fn is None:
            self.gamma, self.lam = 1.0, 1.0           # nstep_target == 1: no discounted term is ever formed
        elif hasattr(fn, "gamma") and hasattr(fn, "lam"):
            self.gamma, self.lam = float(fn.gamma), float(fn.lam)
        else:
            raise ValueError("DeviceOnlineHistory evaluates the GAE(lambda) return of training/a2c.py on the GPU and "
                             "needs a discount_function that carries .gamma and .lam")
        from rltime_amd import _lib
        _lib.require_gpu()
        self.max_delayed_steps, self.fixed_target = max_delayed_steps, fixed_target
        self.plan = OnlinePlan(self.nstep_train, max_delayed_steps)
        self.capacity = 0
        self._rings = None
        self._served = []              # env ids in the order the last batch took them (tests)
        # the sink side (a fused actor configures it): ring handle, floats of policy output per transition, the device
        # word counting the vector steps stored and what the host knows it to hold, discards not yet reported
        self._h, self._policy_f32, self._fused = None, 0, False
        self._head_word, self._word_host, self._pending_discards = None, 0, 0

    def _base_init(self, nstep_target, nstep_train, prefix_steps=0, discount_function=None, state_store=None):
        assert nstep_target == 1 or discount_function is not None, \
            "History buffer must get a 'discount_function' for nstep_target>1"
        self.nstep_target, self.nstep_train, self.prefix_steps = nstep_target, nstep_train, prefix_steps
        self.discount_function = discount_function
        self.state_store = state_store

    @property
    def last_env(self):
        return self.plan.last_env

    # -- feeding ----------------------------------------------------------------------------
    def _configure(self, samples, step):
        frames = step["frames"]
        if "extra" in step or isinstance(samples.example_state["x"], (tuple, list)):
            raise ValueError("DeviceOnlineHistory: extra-feature observations are not supported on the device path")
        lay = self._layout = _Layout(samples.example_state)
        if lay.recurrent:
            if "state" not in step or "initials" not in step or not lay.has_initials:
                raise ValueError("DeviceOnlineHistory: the vector steps of a recurrent policy must carry both its packed "
                                 "`state` [E, S] and its `initials` [E]")
            state, initials = step["state"], step["initials"]
            if tuple(state.shape) != (samples.num_envs, lay.state_f32) or state.dtype != torch.float32:
                raise ValueError("DeviceOnlineHistory: the vector step's state is %s %s, the stored pytree holds float32 [%d, %d]"
                                 % (state.dtype, tuple(state.shape), samples.num_envs, lay.state_f32))
            if tuple(initials.shape) != (samples.num_envs,) or initials.dtype != torch.float32:
                raise ValueError("DeviceOnlineHistory: the vector step's initials are %s %s, not float32 [%d]"
                                 % (initials.dtype, tuple(initials.shape), samples.num_envs))
        elif "state" in step or "initials" in step or lay.has_initials:
            raise ValueError("DeviceOnlineHistory: the vector steps carry a recurrent state or initials that the stored "
                             "pytree has no recurrent layer for")
        self.num_envs, self.env_base = samples.num_envs, samples.env_base
        self._obs_shape, self._obs_dtype = tuple(frames.shape[1:]), frames.dtype
        self._obs_bytes = int(np.prod(self._obs_shape)) * frames.element_size()
        self._device = frames.device
        self._head_word = torch.zeros(1, dtype=torch.int64, device=self._device)
        # the action dtype and trailing shape of the first vector step: int32 [E] (Discrete) or float32 [E, D] (Box), kept in
        # the rings as `_action_words` opaque 4-byte words per transition
        actions = step["actions"]
        self._action_shape = tuple(actions.shape[1:])
        self._action_dtype = torch.float32 if self._action_shape else torch.int32
        self._action_words = int(np.prod(self._action_shape)) if self._action_shape else 1
        if (self._action_shape and actions.dtype != torch.float32) or not 1 <= self._action_words <= 16:
            raise ValueError("DeviceOnlineHistory: actions are integers [E] or float32 [E, D] with D <= 16, not %s %s"
                             % (actions.dtype, tuple(actions.shape)))

    @staticmethod
    def _next_capacity(need, capacity, nstep_train, max_delayed_steps):
        """Doubling, at least a training window and the step before it, at most what can ever be live."""
        return min(max(need, 2 * capacity, nstep_train + 1), max(max_delayed_steps + 1, need))

    def _grow(self, need, written):
        """Rings of `need` or more vector steps, at most max_delayed_steps + 1; the `written` steps already stored keep
        their slot number modulo the new capacity."""
        cap = self._next_capacity(need, self.capacity, self.nstep_train, self.max_delayed_steps)
        E, dev = self.num_envs, self._device
        new = {"obs": torch.empty((cap, E, self._obs_bytes), dtype=torch.uint8, device=dev),
               "actions": torch.empty((cap, E) + self._action_shape, dtype=self._action_dtype, device=dev),
               "rewards": torch.empty((cap, E), dtype=torch.float32, device=dev),
               "dones": torch.empty((cap, E), dtype=torch.uint8, device=dev),
               "policy": torch.empty((cap, E, 2), dtype=torch.float32, device=dev)}
        if self._layout.recurrent:
            new["state"] = torch.empty((cap, E, self._layout.state_f32), dtype=torch.float32, device=dev)
            new["initials"] = torch.empty((cap, E), dtype=torch.float32, device=dev)
        if self._rings is not None:
            live = np.arange(max(0, written - self.capacity), written)
            if len(live):
                src = torch.as_tensor(live % self.capacity, device=dev)
                dst = torch.as_tensor(live % cap, device=dev)
                for k, ring in self._rings.items():
                    new[k][dst] = ring[src]
        self._rings, self.capacity = new, cap
        if self._h is not None:
            self._h.renew()

    # -- the fused acting step's sink ---------------------------------------------------------
    def configure(self, example_state, num_envs, env_base=0, policy_f32=2):
        """The fused actor's set-up call, before its first vector step: the shapes the generic route learns from its first
        DeviceSamples come from the example next_state pytree.  Discrete actions, no extras."""
        if policy_f32 != 2:
            raise ValueError("DeviceOnlineHistory stores the [log-probability | value] pair of every transition: policy_f32 "
                             "must be 2, not %r" % (policy_f32,))
        x = example_state["x"]
        if isinstance(x, (tuple, list)):
            raise ValueError("DeviceOnlineHistory: extra-feature observations are not supported on the device path")
        x = np.asarray(x)
        lay = _Layout(example_state)
        if lay.recurrent and not lay.has_initials:
            raise ValueError("DeviceOnlineHistory: a recurrent policy's stored state must carry `initials`")
        obs_dtype = torch.from_numpy(np.zeros(0, x.dtype)).dtype
        if self._head_word is None:
            self._layout = lay
            self.num_envs, self.env_base = int(num_envs), int(env_base)
            self._obs_shape, self._obs_dtype, self._obs_bytes = tuple(x.shape), obs_dtype, int(x.nbytes)
            self._device = torch.device("cuda", torch.cuda.current_device())
            self._action_shape, self._action_dtype, self._action_words = (), torch.int32, 1
            self._head_word = torch.zeros(1, dtype=torch.int64, device=self._device)
        elif (self.num_envs, self.env_base, self._obs_shape, self._obs_dtype, self._action_shape, self._layout.state_f32) != \
                (int(num_envs), int(env_base), tuple(x.shape), obs_dtype, (), lay.state_f32):
            raise ValueError("DeviceOnlineHistory: the fused actor's vector steps do not match the ones already stored")
        self._policy_f32, self._fused = 2, True
        if self._h is None:
            self._h = _RingHandle()

    def supports_planned_ingest(self):
        return self._h is not None

    def _env_ids(self):
        return range(self.env_base, self.env_base + self.num_envs)

    def _sync_word(self, steps):
        """The device word := `steps` where the host knows it to hold something else (vector steps that came through
        `update`, which moves no word)."""
        if self._word_host != steps:
            self._head_word.fill_(steps)
            self._word_host = steps

    def _append(self, k, frames, actions, rewards, dones, state, initials, policy):
        from rltime_amd._lib import lib, check, ptr as p, stream
        E, S, r = self.num_envs, self._layout.state_f32 if self._layout.recurrent else 0, self._rings
        if self._action_shape:
            raise ValueError("DeviceOnlineHistory: Box actions are fed through update(DeviceSamples), not the fused step")
        if policy is None or tuple(policy.shape) != (E, 2) or policy.dtype != torch.float32 or policy.stride(1) != 1:
            raise ValueError("DeviceOnlineHistory: every vector step carries its float32 [E, 2] = [log-probability | value] block")
        if S and (state is None or initials is None or tuple(state.shape) != (E, S) or tuple(initials.shape) != (E,)):
            raise ValueError("DeviceOnlineHistory: the vector steps of a recurrent policy must carry both its packed "
                             "`state` [E, S] and its `initials` [E]")
        if not S and (state is not None or initials is not None):
            raise ValueError("DeviceOnlineHistory: the vector steps carry a recurrent state or initials that the stored "
                             "pytree has no recurrent layer for")
        dense = [frames, actions, rewards, dones] + ([state, initials] if S else [])
        if frames.numel() * frames.element_size() != E * self._obs_bytes or not all(t.is_contiguous() for t in dense) or \
                (actions.dtype, rewards.dtype, dones.dtype) != (torch.int32, torch.float32, torch.uint8) or \
                any(tuple(t.shape) != (E,) for t in (actions, rewards, dones)) or (S and state.dtype != initials.dtype) or \
                (S and state.dtype != torch.float32):
            raise ValueError("DeviceOnlineHistory: a vector step is contiguous frames [E, ...], int32 actions, float32 rewards "
                             "and uint8 dones [E]")
        check(lib.mirl_online_append(E, self.capacity, p(self._head_word), int(k), self._obs_bytes, p(frames), p(actions),
                                     p(rewards), p(dones), p(policy), policy.stride(0), S, p(state) if S else None,
                                     p(initials) if S else None, p(r["obs"]), p(r["actions"]), p(r["rewards"]), p(r["dones"]),
                                     p(r["policy"]), p(r["state"]) if S else None, p(r["initials"]) if S else None, stream()),
              "mirl_online_append")

    def _advance(self, steps):
        from rltime_amd._lib import lib, check, ptr as p, stream
        check(lib.mirl_online_advance(p(self._head_word), int(steps), stream()), "mirl_online_advance")

    def update_batch(self, frames, actions, rewards, dones, extra=None, state=None, initials=None, policy=None, env_ids=None,
                     transient=False, newest_plane_only=False):
        """One vector step from the fused step's static buffers: the host bookkeeping, then the append launch at the
        device head word (k = 0) and the advance by one."""
        if extra is not None:
            raise ValueError("DeviceOnlineHistory: extra-feature observations are not supported on the device path")
        if self._h is None:
            raise ValueError("DeviceOnlineHistory.update_batch needs configure() first")
        self._pending_discards += self.plan.feed(self._env_ids())
        if self.plan.live_steps() > self.capacity:
            self._grow(self.plan.live_steps(), self.plan.head - 1)
        self._sync_word(self.plan.head - 1)
        self._append(0, frames, actions, rewards, dones, state, initials, policy)
        self._advance(1)
        self._word_host = self.plan.head

    def plan_ingest(self, iters, num_envs):
        """The host side of `iters` vector steps ahead of their launches: feeds the plan, grows the rings to hold what is
        then live, keeps the discards for the next update().  ingest_planned(k) for k = 0 .. iters - 1 and
        finish_planned(iters) follow, possibly as one captured graph."""
        if num_envs != self.num_envs:
            raise ValueError("DeviceOnlineHistory: every vector step must cover the same envs")
        before = self.plan.head
        for _ in range(iters):
            self._pending_discards += self.plan.feed(self._env_ids())
        if self.plan.live_steps() > self.capacity:
            self._grow(self.plan.live_steps(), before)
        self._sync_word(before)
        self._word_host = self.plan.head          # (finish_planned moves the word there)

    def ingest_planned(self, k, frames, actions, rewards, dones, extra=None, state=None, initials=None, policy=None):
        if extra is not None:
            raise ValueError("DeviceOnlineHistory: extra-feature observations are not supported on the device path")
        self._append(k, frames, actions, rewards, dones, state, initials, policy)

    def finish_planned(self, iters):
        """The last node of a rollout: the head word moves past its `iters` steps."""
        self._advance(iters)

    def update(self, samples):
        """Appends the DeviceSamples' vector steps to the rings -> {"discarded_steps": n} (online_history.py:61-73).  Steps
        the fused actor wrote itself (fast_step.IngestedSamples) are only accounted: the discards since the last call."""
        if getattr(samples, "ingested", False):
            discarded, self._pending_discards = self._pending_discards, 0
            return {"discarded_steps": discarded}
        if not hasattr(samples, "vector_steps"):
            raise TypeError("DeviceOnlineHistory takes the device actor's DeviceSamples (whole vector steps); per-env "
                            "sample dicts belong to OnlineHistoryBuffer")
        discarded = 0
        for step in samples.vector_steps:
            if self._head_word is None:
                self._configure(samples, step)
            if samples.num_envs != self.num_envs or samples.env_base != self.env_base:
                raise ValueError("DeviceOnlineHistory: every vector step must cover the same envs")
            discarded += self.plan.feed(range(self.env_base, self.env_base + self.num_envs))
            if self.plan.live_steps() > self.capacity:
                self._grow(self.plan.live_steps(), self.plan.head - 1)
            slot = (self.plan.head - 1) % self.capacity
            r = self._rings
            r["obs"][slot].copy_(step["frames"].reshape(self.num_envs, -1).view(torch.uint8))
            r["actions"][slot].copy_(step["actions"])
            r["rewards"][slot].copy_(step["rewards"])
            r["dones"][slot].copy_(step["dones"])
            r["policy"][slot].copy_(step["policy"])
            if self._layout.recurrent:
                r["state"][slot].copy_(step["state"])
                r["initials"][slot].copy_(step["initials"])
        if self._fused:
            self._sync_word(self.plan.head)      # a fused actor feeds this history too: its head word follows every route
        return {"discarded_steps": discarded}

    def needed_feed_count(self, mbatch_size, num_envs):
        """online_history.py:75-79: feed one vector step whenever no batch can be formed.  For a fused actor — whose
        acting call is one graph launch however many steps it covers — the whole vector steps still missing are asked for
        at once: with synchronous envs and no training in between, the same env stream as one step at a time."""
        if self.plan.sequences_ready() >= mbatch_size:
            return None
        if self._fused:
            steps = self.plan.steps_until_ready(mbatch_size, self._env_ids())
            return num_envs * (steps or 1)
        return num_envs

    # -- training batches --------------------------------------------------------------------
    def get_train_data(self, mbatch_size, train_progress=None):
        """online_history.py:81-120: `mbatch_size` sequences of nstep_train consecutive transitions, round-robin over
        the env ids, each removed as soon as it is handed out.  None = feed more.  The batch has the host class's keys
        and (T, B, ...) layout, as device tensors."""
        from rltime_amd._lib import lib, check, ptr as p, stream
        served = self.plan.serve(mbatch_size)
        if served is None:
            return None
        self._served = [env for env, _, _ in served]
        T, B, E, cap, dev = self.nstep_train, mbatch_size, self.num_envs, self.capacity, self._device
        rows = np.array([(env - self.env_base, start % cap, own) for env, start, own in served], dtype=np.int32)
        assert rows[:, 0].min() >= 0 and rows[:, 0].max() < E and cap >= T + 1
        plan = torch.from_numpy(rows).to(dev, non_blocking=True)
        f32 = lambda: torch.empty((T, B), dtype=torch.float32, device=dev)      # noqa: E731
        returns, nsteps, masks, logp, values = f32(), f32(), f32(), f32(), f32()
        actions = torch.empty((T, B) + self._action_shape, dtype=self._action_dtype, device=dev)
        obs = torch.empty((2, T, B, self._obs_bytes), dtype=torch.uint8, device=dev)
        r = self._rings
        pol = r["policy"]
        args = (T, B, E, cap, self.nstep_target, self.gamma, self.lam, self._obs_bytes, p(plan), p(r["obs"]),
                p(r["actions"]), p(r["rewards"]), p(r["dones"]), p(pol), p(pol.view(-1)[1:]), 2,
                p(returns), p(nsteps), p(masks), p(actions), p(logp), p(values), p(obs[0]), p(obs[1]))
        lay = self._layout
        state = initials = None
        if lay.recurrent:             # the same kernel body also moving the recurrent state and the initials flag of every row
            state = torch.empty((2, T, B, lay.state_f32), dtype=torch.float32, device=dev)
            initials = torch.empty((2, T, B), dtype=torch.float32, device=dev)
            check(lib.mirl_online_window_rec(*args, self._action_words, p(r["state"]), p(r["initials"]), lay.state_f32,
                                             p(state[0]), p(state[1]), p(initials[0]), p(initials[1]), stream()),
                  "mirl_online_window_rec")
        elif self._action_shape:      # Box actions: the same kernel body moving `_action_words` words per transition
            check(lib.mirl_online_window_box(*args, self._action_words, stream()), "mirl_online_window_box")
        else:
            check(lib.mirl_online_window(*args, stream()), "mirl_online_window")
        shaped = obs.view(self._obs_dtype).reshape((2, T, B) + self._obs_shape)

        def tree(i):
            out, at, rec = {"x": shaped[i]}, 0, dict(lay.recurrent)
            for k in lay.layer_keys:
                out[k] = {}
                for name, size, shape in rec.get(k, ()):
                    out[k][name] = state[i][..., at:at + size].reshape((T, B) + shape)
                    at += size
                if k in rec:
                    out[k]["initials"] = initials[i]
            return out
        return {"states": tree(0), "target_states": tree(1), "returns": returns, "nsteps": nsteps,
                "target_masks": masks, "policy_outputs": {"actions": actions, "action_log_probs": logp, "values": values},
                "extra_data": {}}

    def update_losses(self, indices, losses):
        pass

    def close(self):
        self._rings = None
        if self._h is not None:
            self._h.renew()

