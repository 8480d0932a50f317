"""A2C trainer with GAE returns (reference rltime/training/torch/a2c.py:6-141).

Two paths.  CPU policies (cartpole_a2c.json / cartpole_ppo.json) run the reference's plain-torch expression on the host
history.  With the device-resident actor and a GPU policy the rollouts stay on the device (history/online_device.py) and
the loss with both gradients is one launch of csrc/actor_critic.hip (training/qops.py ac_loss)."""
from .torch_trainer import TorchTrainer
from rltime_amd.general.utils import anneal_value
from rltime_amd.policies.actor_critic import ActorCriticPolicy


class A2C(TorchTrainer):
    def _train(self, entropy_factor, entropy_anneal=None, vf_coef=1.0, advlam=1.0, adv_norm=False,
               history_mode={"type": "online"}, **kwargs):
        """a2c.py:21-46: on-policy history by default."""
        self.entropy_factor, self.entropy_anneal = entropy_factor, entropy_anneal
        self.vf_coef, self.advlam, self.adv_norm = vf_coef, advlam, adv_norm
        self._check_actor_critic_config(kwargs, history_mode)
        super()._train(history_mode=history_mode, **kwargs)

    def _on_device(self):
        """Rollouts on the device: the device-resident actor with a policy on the GPU."""
        return bool(getattr(self.actors, "_device_mode", False)) and self.policy.is_cuda()

    def _check_actor_critic_config(self, kwargs, history_mode):
        """What the actor-critic trainers do not cover is refused here, before optimizer and history are built."""
        for key in ("graph_learner_step", "skip_invalid_steps", "overlap_acting"):
            if kwargs.get(key):
                raise ValueError("%s is not supported with an actor-critic trainer (A2C / PPO)" % key)
        if getattr(self, "eval_episodes", 0):
            raise ValueError("eval_episodes is not supported with an actor-critic trainer (A2C / PPO)")
        if not hasattr(self.actors.get_spaces()[1], "n") and history_mode.get("type") != "online":
            raise ValueError("a Box action space needs history_mode type 'online', not %r: the replay histories store one "
                             "integer action per transition" % (history_mode.get("type"),))
        if not self._on_device():
            return
        dp = getattr(self, "data_parallel", None)
        if dp is not None and getattr(dp, "active", True):
            raise ValueError("A2C / PPO on the device path do not run under a process group")
        why = self.policy.why_not_on_device()
        if why is not None:
            raise ValueError("A2C / PPO: %s" % why)
        if history_mode.get("type") != "online":
            raise ValueError("A2C / PPO on the device path need history_mode type 'online', not %r" % (history_mode.get("type"),))
        if not history_mode.get("args", {}).get("fixed_target", True):
            raise ValueError("fixed_target=False is not supported on the device path: its targets look past the window")
        if kwargs.get("burn_in_timesteps"):
            raise ValueError("burn_in_timesteps is not supported with the device online history: it has no prefix steps")
        if kwargs.get("rnn_bootstrap"):
            raise ValueError("rnn_bootstrap is not supported with the device online history: its n-steps are not fixed")
        if self.policy.is_recurrent():
            # whole sequences per minibatch (multi_step_trainer.py:47-68 asserts the same in the middle of training)
            T = kwargs["nstep_train"]
            rnn = kwargs.get("rnn_steps_train") or T
            seqs = kwargs.get("mbatch_size") or self.actors.get_env_count()
            parts = kwargs.get("minibatches", 1)
            if T % rnn:
                raise ValueError("a recurrent policy trains on whole sequences: nstep_train (%d) must be a multiple of "
                                 "rnn_steps_train (%d)" % (T, rnn))
            if (seqs * T) % parts or (seqs * T // parts) % T:
                raise ValueError("a recurrent policy trains on whole sequences: every minibatch must hold a whole number of "
                                 "the batch's %d sequences of nstep_train = %d steps, so minibatches (%d) must divide %d"
                                 % (seqs, T, parts, seqs))

    def _init_history_buffer(self, mode, *args, **kwargs):
        """The reference's history_mode {"type": "online"} resolves to the device class when the rollouts are on the
        device; the host class stays for everything else."""
        if self._on_device():
            mode = dict(mode, type="online_device")
        super()._init_history_buffer(mode, *args, **kwargs)

    @staticmethod
    def create_policy(**kwargs):
        return ActorCriticPolicy.create(**kwargs)

    def _get_discount_function(self, gamma):
        """a2c.py:48-66: the k-th term of a truncated GAE(lambda) return, from the reward and the acting-time value
        estimate of step k; lambda = 1 gives gamma^k r.  (The bootstrap and the -V(s_t) are added by the trainer.)
        `.gamma` / `.lam` let the device history evaluate the same return on the GPU."""
        lam = self.advlam

        def discount(nstep, reward, policy_output):
            v = policy_output["values"]
            return (gamma ** nstep) * (lam ** (nstep - 1)) * (v + lam * (reward - v))
        discount.gamma, discount.lam = gamma, lam
        return discount

    def _discount_bootstrap_target_value(self, target_values, nsteps):
        """a2c.py:68-71."""
        return (self.gamma ** nsteps) * (self.advlam ** (nsteps - 1)) * target_values

    def _get_bootstrap_target_value(self, target_states, timesteps):
        """a2c.py:73-82: V(target state) from the target policy (normally the online one)."""
        return self.target_policy.get_state_value(target_states, timesteps=timesteps)

    def _calc_entropy_factor(self):
        return anneal_value(self.entropy_factor, self.get_train_progress(), self.entropy_anneal)

    def _calc_action_gain(self, action_log_probs, advantages, org_policy_outputs):
        """a2c.py:90-99: vanilla advantage actor-critic."""
        assert action_log_probs.shape == advantages.shape
        return (action_log_probs * advantages).mean()

    _fused_gain = _calc_action_gain       # the gain _fused_loss_args describes to the kernel

    def _fused_loss_args(self, policy_outputs):
        """(old log-probabilities, clip value) of the fused loss: the A2C gain takes neither."""
        return None, None

    def _fused_loss_ok(self):
        """A GPU policy the device path covers (Categorical or Normal head), and an action gain the kernel knows (a plugin
        trainer that overrides _calc_action_gain keeps the plain-torch expression)."""
        pol = self.policy
        known = type(self)._calc_action_gain is getattr(type(self), "_fused_gain", None)
        return known and pol.is_cuda() and hasattr(pol, "why_not_on_device") and pol.why_not_on_device() is None

    def _compute_grads_fused(self, states, targets, policy_outputs, timesteps):
        """The same loss as below with forward and backward in one launch (csrc/actor_critic.hip mirl_ac_loss); the four
        logged scalars come out of the launch's stats block."""
        from . import qops
        mk = self.policy.make_tensor
        old, clip = self._fused_loss_args(policy_outputs)
        common = dict(old_log_probs=old, vf_coef=self.vf_coef, entropy_factor=self._calc_entropy_factor(), clip_value=clip,
                      adv_norm=self.adv_norm)
        if self.policy.has_normal_head():
            # Box actions: mirl_ac_loss_normal, with the gradient of the state-independent log-std out of the same launch
            mean, logstd, values = self.policy.get_mean_logstd_and_state_value(states, timesteps)
            assert targets.dim() == 1 and targets.shape == values.shape
            loss, stats = qops.ac_loss_normal(mean, logstd, values, mk(policy_outputs["actions"]), targets,
                                              mk(policy_outputs["values"]), **common)
        else:
            logits, values = self.policy.get_logits_and_state_value(states, timesteps)
            assert targets.dim() == 1 and targets.shape == values.shape
            loss, stats = qops.ac_loss(logits, values, mk(policy_outputs["actions"]), targets, mk(policy_outputs["values"]), **common)
        loss.backward()
        log = self.value_log.log
        stats = stats.detach()
        log("state_value_mean", stats[4], group="train")
        log("value_loss", stats[1], group="train")
        log("policy_loss", stats[2], group="train")
        log("policy_entropy", stats[3], group="train")

    def _compute_grads(self, states, targets, policy_outputs, extra_data, timesteps):
        """a2c.py:101-141: value MSE * vf_coef - action gain - entropy bonus; advantages against the ACTING-time
        value estimates, optionally normalised."""
        if self._fused_loss_ok():
            return self._compute_grads_fused(states, targets, policy_outputs, timesteps)
        log_probs, values, entropy = self.policy.evaluate_actions(states, timesteps, policy_outputs["actions"])
        entropy = entropy.mean()
        assert log_probs.dim() == 1 and targets.dim() == 1
        baseline = self.policy.make_tensor(policy_outputs["values"])
        assert baseline.shape == targets.shape == values.shape
        advantages = targets - baseline
        if self.adv_norm:
            advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-5)
        gain = self._calc_action_gain(log_probs, advantages, policy_outputs)
        value_loss = (targets - values).pow(2).mean()
        loss = value_loss * self.vf_coef - gain - self._calc_entropy_factor() * entropy
        loss.backward()
        log = self.value_log.log
        log("state_value_mean", values.mean().item(), group="train")
        log("value_loss", value_loss.item(), group="train")
        log("policy_loss", -gain.item(), group="train")
        log("policy_entropy", entropy.item(), group="train")
