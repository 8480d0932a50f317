"""ActorCriticPolicy and its action-distribution heads (reference
rltime/policies/torch/actor_critic.py:9-107, policies/torch/distributions/{categorical,normal}.py).

Used by the A2C / PPO trainers.  On the CPU (BASELINE configs[0], `cartpole_ppo.json`) everything here is plain PyTorch;
on the GPU a Categorical policy hands its raw logits and values to the kernels of csrc/actor_critic.hip
(`actor_head_ac_raw` for the acting step, `get_logits_and_state_value` for the fused loss), a Normal policy its means,
log-std and values (`actor_head_normal_raw`, `get_mean_logstd_and_state_value`)."""
import numpy as np
import torch
import torch.nn as nn

from .torch_policy import TorchPolicy
from rltime_amd.models.torch.utils import linear
from rltime_amd.spaces import is_tuple_space


class CategoricalHead(nn.Module):
    """distributions/categorical.py:8-20: one action out of action_space.n."""

    def __init__(self, action_space, input_size):
        super().__init__()
        self.logits_layer = linear(input_size, action_space.n)

    def forward(self, x):
        return torch.distributions.Categorical(logits=self.logits_layer(x))


class NormalHead(nn.Module):
    """distributions/normal.py:9-36: independent Gaussians over a Box action, state-independent log-std."""

    def __init__(self, action_space, input_size):
        super().__init__()
        self.actions_shape = tuple(action_space.shape)
        flat = int(np.prod(self.actions_shape))
        self.mean_layer = linear(input_size, flat)
        self.logstd = nn.Parameter(torch.zeros(flat))

    def forward(self, x):
        mean = self.mean_layer(x)
        std = self.logstd.exp().expand_as(mean)
        shape = (x.shape[0],) + self.actions_shape
        return torch.distributions.Normal(mean.view(shape), std.view(shape))


def distribution_head(action_space):
    """distributions/__init__.py:6-16 by duck type (gym is not a dependency here): `.n` = Discrete, a shaped box otherwise."""
    if hasattr(action_space, "n"):
        return CategoricalHead
    if not is_tuple_space(action_space) and len(getattr(action_space, "shape", ())) > 0:
        return NormalHead
    raise ValueError("Unsupported action_space, there is no distribution class available for: %s" % type(action_space))


class ActorCriticPolicy(TorchPolicy):
    def __init__(self, model_config, observation_space, action_space, critic_separate_model=False):
        """actor_critic.py:10-35."""
        super().__init__(model_config, observation_space)
        self.value_model = self._create_model_from_config(model_config, observation_space) if critic_separate_model else None
        self.actor = distribution_head(action_space)(action_space, self.model.out_size)
        self.critic = linear(self.model.out_size, 1)

    def get_dist_and_state_value(self, x, timesteps):
        """actor_critic.py:95-107."""
        features = self.model(x, timesteps)["output"]
        dist = self.actor(features)
        if self.value_model is not None:
            features = self.value_model(x, timesteps)["output"]
        return dist, self.critic(features).squeeze(-1)

    def get_state_value(self, inp, timesteps):
        """actor_critic.py:73-80."""
        model = self.value_model if self.value_model is not None else self.model
        return self.critic(model(inp, timesteps)["output"]).squeeze(-1)

    def why_not_on_device(self):
        """What keeps this policy off the device actor-critic path (csrc/actor_critic.hip), or None.  (A recurrent model is
        covered: the raw-output getters below pass the state pytree through the model, and the device history keeps the
        recurrent state of every row.)"""
        if self.value_model is not None:
            return "critic_separate_model is not supported on the device path"
        if isinstance(self.actor, NormalHead):
            if self.actor.logstd.numel() > 16:
                return "more than 16 action components are not supported on the device path"
        elif self.actor.logits_layer.out_features > 64:
            return "more than 64 actions are not supported on the device path"
        return None

    def has_normal_head(self):
        return isinstance(self.actor, NormalHead)

    def get_mean_logstd_and_state_value(self, inp, timesteps):
        """The Normal head's raw means (rows, D), its log-std parameter (D,) and the state values (rows,): what the fused
        loss (training/qops.py ac_loss_normal) differentiates."""
        features = self.model(inp, timesteps)["output"]
        return self.actor.mean_layer(features), self.actor.logstd, self.critic(features).squeeze(-1)

    def actor_head_normal_raw(self, inp, timesteps):
        """No-grad (means, logstd, values) of one acting step for the Normal sampling-head kernel (acting/actor.py)."""
        why = self.why_not_on_device()
        if why is not None:
            raise ValueError(why)
        with torch.no_grad():
            mean, logstd, values = self.get_mean_logstd_and_state_value(inp, timesteps)
        return mean.contiguous(), logstd.detach().contiguous(), values.contiguous()

    def get_logits_and_state_value(self, inp, timesteps):
        """The Categorical head's raw logits (rows, A) and the state values (rows,): what the fused loss
        (training/qops.py ac_loss) differentiates."""
        features = self.model(inp, timesteps)["output"]
        return self.actor.logits_layer(features), self.critic(features).squeeze(-1)

    def actor_head_ac_raw(self, inp, timesteps):
        """No-grad (logits, values) of one acting step for the sampling-head kernel (acting/actor.py _select)."""
        why = self.why_not_on_device()
        if why is not None:
            raise ValueError(why)
        if self.has_normal_head():
            raise ValueError("actor_head_ac_raw is the Categorical head's; a Normal head acts through actor_head_normal_raw")
        with torch.no_grad():
            logits, values = self.get_logits_and_state_value(inp, timesteps)
        return logits.contiguous(), values.contiguous()

    @staticmethod
    def _joint(log_probs):
        # a multi-dimensional action's log-probability is the sum over its components (actor_critic.py:57-58, :88-89)
        return log_probs.sum(-1) if log_probs.dim() == 2 else log_probs

    def actor_predict(self, inp, timesteps, force_best=False):
        """actor_critic.py:37-71: sampled (or arg-max) actions with the log-probabilities and value estimates
        the trainer needs later."""
        if force_best and not isinstance(self.actor, CategoricalHead):
            # (the reference's arg-max of dist.logits fails for a Normal distribution too: actor_critic.py:50-53)
            raise ValueError("force_best is not supported for the Normal (continuous) action head: it has no greedy mode")
        with torch.no_grad():
            dist, values = self.get_dist_and_state_value(inp, timesteps)
            actions = dist.logits.argmax(dim=-1) if force_best else dist.sample()
            log_probs = self._joint(dist.log_prob(actions))
        return {"actions": actions.cpu().numpy(), "action_log_probs": log_probs.cpu().numpy(),
                "values": values.cpu().numpy()}

    def evaluate_actions(self, inp, timesteps, actions):
        """actor_critic.py:82-93 -> (log-probabilities of `actions`, state values, entropy)."""
        dist, values = self.get_dist_and_state_value(inp, timesteps)
        return self._joint(dist.log_prob(self.make_tensor(actions))), values, dist.entropy()
