"""Distributional DQN, C51 (reference rltime/training/torch/dist_dqn.py:10-142) with the
target projection and the loss on fused HIP kernels (rltime_amd/csrc/c51.hip).

The reference projects with Tz_j = (r + mask * gamma^n) * z_j, not the paper's
r + mask * gamma^n * z_j, and drops the mass of every atom whose b = (Tz - vmin) / dz
lands on an integer (l == u: both of its shares are zero) — a terminal row with reward 0
gets an all-zero target.  Both are reproduced by default; projection="paper" (not a
reference argument) selects the paper's formula, with the whole mass of such an atom
kept in its bin."""
import torch

from .dqn import DQN
from . import qops
from rltime_amd.policies.dist_dqn import DistDQNPolicy


class DistDQN(DQN):
    def _train(self, *args, loss_mode="crossentropy", projection="reference", **kwargs):
        """dist_dqn.py:21-24: cross-entropy by default, mse / huber of p - t on request."""
        assert projection in ("reference", "paper"), "%s is not a C51 projection" % projection
        assert not kwargs.get("vf_scale_epsilon"), "DistDQN does not support value function rescaling"
        hist_args = (kwargs.get("history_mode") or {}).get("args", {}) or {}
        if hist_args.get("acting_priority_init"):
            raise ValueError("acting_priority_init is not supported by dist_dqn: its acting-time priority is the "
                             "scalar-Q TD error, not a distributional loss")
        self.projection = projection
        super()._train(*args, loss_mode=loss_mode, **kwargs)

    def _check_loss_mode(self, loss_mode):
        assert loss_mode in ("crossentropy", "huber", "mse"), "%s is not a valid dist_dqn loss mode" % loss_mode

    @staticmethod
    def create_policy(**kwargs):
        return DistDQNPolicy.create(**kwargs)

    def calc_target_values(self, returns, target_states, target_masks, nsteps, timesteps):
        """dist_dqn.py:30-97: the forwards in the reference's order (target net, then the online net for double-Q,
        always through the full predict: the softmax follows the dueling combine), then one kernel for selection,
        target softmax and projection."""
        with torch.no_grad():
            assert not self.vf_scale_epsilon, "DistDQN does not support value function rescaling"
            lt = self.target_policy.predict(target_states, timesteps=timesteps)
            ls = lt if not self.double_q else self.policy.predict(target_states, timesteps=timesteps)
            pol, mk = self.policy, self.policy.make_tensor
            return qops.q_target_c51(lt, ls, pol.support, mk(returns), mk(nsteps), mk(target_masks), self.gamma,
                                     pol.vmin, pol.vmax, getattr(self, "projection", "reference"))

    def _get_bootstrap_target_value(self, target_states, timesteps):
        raise NotImplementedError("dist_dqn bootstraps whole distributions: see calc_target_values")

    def _compute_grads(self, states, targets, policy_outputs, extra_data, timesteps):
        """dist_dqn.py:99-142."""
        logits = self.policy.predict(states, timesteps)
        actions = self.policy.make_tensor(policy_outputs["actions"]).long()
        assert logits.dim() == 3 and logits.shape[-1] == self.policy.num_atoms
        assert actions.shape == logits.shape[:1] and targets.shape == (logits.shape[0], logits.shape[2])
        loss, report = qops.c51_loss(logits, actions, targets, self._weights(extra_data), self.loss_mode,
                                     self.huber_kappa, timesteps, self.loss_aggregation, self.loss_timestep_aggregation)
        loss.backward()
        self._report_losses_if_needed(report, extra_data)
        self.value_log.log("qloss", loss.detach(), group="train")
