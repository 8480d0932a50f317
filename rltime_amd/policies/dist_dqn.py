"""DistDQNPolicy (reference rltime/policies/torch/dist_dqn.py:6-33): C51's categorical
distribution over `num_atoms` fixed atoms per action."""
import torch

from .dqn import DQNPolicy


class DistDQNPolicy(DQNPolicy):
    def __init__(self, *args, num_atoms=51, vmin=-10, vmax=10, **kwargs):
        self.num_atoms = num_atoms
        self.vmin = vmin
        self.vmax = vmax
        super().__init__(*args, **kwargs)
        # dist_dqn.py:17-22: the atoms, a persistent buffer that moves with the module
        self.register_buffer("support", torch.linspace(self.vmin, self.vmax, self.num_atoms))

    def _outputs_per_action(self):
        return self.num_atoms

    def _shape_action_outputs(self, output):
        """(rows, A * Z) -> (rows, A, Z): the atoms on the last axis, the dueling mean over axis 1."""
        return output.view((output.shape[0], -1, self.num_atoms)), 1

    def predict_selection(self, x, timesteps):
        """No advantage-only shortcut: the softmax over atoms follows the dueling combine, so the
        advantage stream's expected values do not rank the actions as Q's do."""
        return self.predict(x, timesteps)

    def _actor_predict_postprocess(self, pred):
        """dist_dqn.py:30-33: expected value of each action's distribution."""
        assert pred.shape[2] == self.num_atoms
        return (torch.nn.functional.softmax(pred, dim=-1) * self.support).sum(2)
