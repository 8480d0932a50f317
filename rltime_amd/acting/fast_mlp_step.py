"""The fused vector step for MLP Q-learning policies on float32 vector observations (cartpole_dqn / cartpole_iqn:
FC(64) -> FC(64), plain or dueling DQN / IQN head), opt-in through acting.extra_args.fused_step (Actor(fused_mlp=True)).

Per vector step the launches are

    env.step_into             1 launch         the device CartPole, into the static observation block
    mirl_actor_pre            1 launch         initials, reward clip, episode statistics, RNG step (H = 0: no carry)
    the sink's ingest         1 copy + 1 launch  the float32 observation as its bytes (history/replay_history.py)
    mirl_act_mlp_fwd          1 launch         csrc/act_mlp.hip: leading layers, quantile draw + cos features + embedding
                                               product, [last FC | value-hidden], outputs, dueling combine, mean over the
                                               quantile rows, first maximum, epsilon-greedy — one workgroup per env

where the generic device path (actor.GraphedStep) replays about a dozen library launches plus PyTorch glue for the
network alone.  Everything around the network is fast_step.FastActingStep's code, inherited unchanged: the pre-step,
the sink protocol, the rollout capture (a whole get_samples call as ONE graph), the Philox keying and the MIRL_ROLLOUT_*
switches.  This class replaces the constructor, `refresh` (the kernel reads TRANSPOSED weight copies, [K][J] row-major,
so that a wave's lanes read consecutive output units; rebuilt once per weight version), `_conv1` (there is no input
layer: a foreign observation is staged into the static input block) and `_body` (the one launch).

FastMlpAcStep is the same step for an actor-critic (A2C / PPO) MLP policy under a Categorical head: mirl_act_mlp_ac_fwd as
the one launch, the [log-probability | value] block where the q-values are, the on-policy history as the sink
(Actor(fused_actor_critic=True), the same config key)."""
import ctypes as C
import os

import numpy as np
import torch

from rltime_amd._lib import lib, check, ptr, stream
from .fast_step import FastActingStep


class FastMlpStep(FastActingStep):
    AC = False                                   # FastMlpAcStep below: the actor-critic head on the same trunk

    @staticmethod
    def _fc_stack(pol):
        """-> the Linears of a model of one to three FC modules of a single Linear + ReLU each, else a string that says what
        is in the way."""
        from rltime_amd.models.torch.modules import FC
        model = pol.model
        layers = list(model.layers)
        if not 1 <= len(layers) <= 3 or not all(isinstance(layer, FC) for layer in layers):
            return "the model is not one to three FC modules"
        if model.extra_input_layer is not None:
            return "the model takes extra features"
        lins = []
        for fc in layers:
            blocks = fc.layers
            if not (fc.fuse_relu and len(blocks) == 1 and len(blocks[0]) == 1):
                return "an FC module is not a single Linear + ReLU"
            lin = blocks[0][0]
            if not (lin.weight.is_cuda and lin.weight.dtype == torch.float32 and lin.bias is not None):
                return "an FC module's Linear is not float32 on the GPU with a bias"
            lins.append(lin)
        return lins

    @staticmethod
    def _mlp_parts(pol):
        """-> (leading Linears, the last layer's Linear, dueling) for a model `_fc_stack` takes, else its reason."""
        lins = FastMlpStep._fc_stack(pol)
        if isinstance(lins, str):
            return lins
        dueling = getattr(pol, "value_layer", None) is not None
        if dueling and pol._fused_tail_layer() is not lins[-1]:
            return "the dueling value stream does not read the last layer's input"
        if pol.out_layer.in_features != lins[-1].out_features or pol.out_layer.bias is None:
            return "the output layer does not read the last FC module"
        return lins[:-1], lins[-1], dueling

    @staticmethod
    def _shape(pol, parts, E, A):
        """The arguments of mirl_act_mlp_supported: (E, O, L, widths, N, D, HID, NO, A)."""
        leading, last, dueling = parts
        iqn = hasattr(pol, "num_sampling_quantiles")
        O = leading[0].in_features if leading else last.in_features
        widths = (C.c_int32 * 2)(*([lin.out_features for lin in leading] + [0, 0])[:2])
        hv = pol.value_hidden_layer.out_features if dueling else 0
        return (E, O, len(leading), widths, pol.num_sampling_quantiles if iqn else 1, int(pol.embedding_dim) if iqn else 0,
                last.out_features + hv, A + (1 if dueling else 0), A)

    @staticmethod
    def why_not(actor, pol=None):
        """None when the step covers this actor's policy and env, else the reason as a string."""
        pol = pol if pol is not None else actor._policy
        try:
            if not getattr(pol, "is_cuda", lambda: False)():
                return "the policy is not on the GPU"
            if not hasattr(actor._action_space, "n"):
                return "the action space is not Discrete"
            if hasattr(pol, "actor_head_ac_raw") or hasattr(pol, "num_atoms") or not hasattr(pol, "actor_head_raw"):
                return "the head is not a plain or dueling DQN / IQN head"
            parts = FastMlpStep._mlp_parts(pol)
            if isinstance(parts, str):
                return parts
            pre = pol.model.layer_pre_processors
            iqn = hasattr(pol, "num_sampling_quantiles")
            if (iqn and set(pre) != {len(pol.model.layers) - 1}) or (not iqn and pre):
                return "the quantile layer is not injected before the last layer"
            space = actor._vec_env.observation_space
            if hasattr(space, "spaces") or str(getattr(space, "dtype", "")) != "float32" or len(tuple(space.shape)) != 1:
                return "the observation space is not a float32 vector"
            if not hasattr(actor._vec_env, "step_device"):
                return "the env does not step on the device"
            expl = actor._exploration
            if expl is not None and not hasattr(expl, "_device_exponents"):
                return "the exploration has no device-side epsilon"
            shape = FastMlpStep._shape(pol, parts, actor._num_envs, actor._action_space.n)
            if shape[1] != int(space.shape[0]):
                return "the first layer does not read the observation"
            if iqn and pol.quantile_layer.in_features != shape[5]:
                return "the quantile layer's input is not the embedding"
            if not lib.mirl_act_mlp_supported(*shape):
                return "mirl_act_mlp_supported refuses the shape (E, O, L, widths, N, D, HID, NO, A) = %r" % (
                    shape[:3] + (list(shape[3])[:shape[2]],) + shape[4:],)
            return None
        except Exception as e:                           # a policy this code does not know: not covered
            return "%s: %s" % (type(e).__name__, e)

    @staticmethod
    def supports(actor):
        """A GPU policy with a Discrete action space, a plain or dueling DQN / IQN head over one to three FC modules of a
        single Linear + ReLU each, IQN injected before the last layer, a float32 [O] observation, an env with
        step_device, epsilon-greedy or greedy, and a shape mirl_act_mlp_supported takes."""
        return FastMlpStep.why_not(actor) is None

    def __init__(self, actor, obs0, need_q=True):
        self.actor = actor
        pol = self.pol = actor._policy
        self.c51, self.ac = False, self.AC
        self.Z = 1
        self.need_q = bool(need_q) or self.ac
        self.leading, self.fc, self.dueling = self._mlp_parts(pol)
        self.lstm = self.cnn = None
        self.iqn = hasattr(pol, "num_sampling_quantiles")
        dev = self.dev = pol.device()
        E = self.E = actor._num_envs
        A = self.A = actor._action_space.n
        self.shape = self._shape(pol, (self.leading, self.fc, self.dueling), E, A)
        _, self.O, self.L, self.widths, self.N, self.D, self.HID, self.NO, _ = self.shape
        # no recurrent layer, no extras: the inherited pre-step, ingest and resume code see empty blocks
        self.H = self.X = self.Xp = self.F = self.K = 0
        self.W = self.fc.in_features
        self.h1 = self.fc.out_features
        f32 = dict(dtype=torch.float32, device=dev)
        self.xh = torch.zeros((E, 0), **f32)
        self.extra = None
        self.c_in = torch.zeros((E, 0), **f32)
        self.h = torch.zeros((E, 0), **f32)
        self.c = torch.zeros((E, 0), **f32)
        self.state_pack = torch.zeros((E, 0), **f32)
        self.initials = torch.ones(E, **f32)
        self.rewards = torch.zeros(E, **f32)
        self.dones = torch.ones(E, dtype=torch.uint8, device=dev)
        self.actions = torch.zeros(E, dtype=torch.int32, device=dev)
        self.qvalues = torch.zeros((E, 2 if self.ac else A), **f32)      # actor-critic: [log-probability | value]
        self.eps = torch.zeros((), dtype=torch.float64, device=dev)
        self.rng_step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.step_no = 0
        self.rng_seed = (int(torch.initial_seed()) ^ (int(actor._base_env_id) << 32) ^ 0xAC7) & 0x7FFFFFFFFFFFFFFF
        if getattr(actor, "_rng_seed", None) is not None:        # an actor with a Philox key of its own (acting/evaluator.py)
            self.rng_seed = int(actor._rng_seed) & 0x7FFFFFFFFFFFFFFF
        # the transposed weight copies the kernel reads ([K][J] row-major), rebuilt by refresh()
        self.lwT = [torch.empty((lin.in_features, lin.out_features), **f32) for lin in self.leading]
        self.fcT = torch.empty((self.W, self.HID), **f32)
        self.fc_b = torch.empty(self.HID, **f32)
        self.outT = torch.zeros((self.HID, self.NO), **f32)      # block-diagonal under a dueling head: the zeros stay
        self.out_b = torch.empty(self.NO, **f32)
        self.wqT = torch.empty((self.D, self.W), **f32) if self.iqn else None
        self.freq = (pol.embedding_range * np.pi).contiguous() if self.iqn else None
        self.taus = torch.zeros(E * self.N, **f32) if self.iqn else None      # a test's tau_source is staged here
        self.in_kernel_taus = self.iqn and getattr(pol, "tau_source", None) is None
        # (an actor-critic policy samples for itself: exploration configs are ignored, as in the reference and in fast_step.py;
        # only the evaluator asks for its fixed epsilon's remap, acting/evaluator.py)
        expl = actor._exploration if (not self.ac or getattr(actor, "_ac_eps_remap", False)) else None
        self.expo = expl._device_exponents(actor._env_ids, dev) if expl is not None else None
        self.eps_min = float(expl.eps_min) if expl is not None else 0.0
        self.last_obs = obs0
        self.trusted_stack = False
        self.tracker = None
        self.graph = None
        env = actor._vec_env
        self.env_into = bool(getattr(env, "supports_step_into", lambda: False)())
        self.env_pre = False                                      # the env step and the pre-step stay two launches
        if hasattr(env, "bind_actions"):
            env.bind_actions(self.actions)       # an env that needs the actions reads them from the head's static buffer
        # the static input block the kernel reads: the env's step_into target where it has one
        self.x_in = torch.empty((E, self.O), **f32)
        if self.env_into:
            self.obs_buf = self.x_in
            self.env_rewards = torch.zeros(E, **f32)
            self.env_dones = torch.zeros(E, dtype=torch.uint8, device=dev)
        self._rollouts = {}
        self.rollout_graphs = os.environ.get("MIRL_ROLLOUT_GRAPH", "1") != "0"
        self.rollout_eager_calls = int(os.environ.get("MIRL_ROLLOUT_EAGER_CALLS", "0"))
        # the reference's first input state: every env starts an episode (actor.py:78-89)
        self.refresh()
        self._pre(torch.zeros(E, **f32), torch.ones(E, dtype=torch.uint8, device=dev), track=False)
        self.example = {"x": obs0[0].cpu().numpy()}
        for i in range(len(pol.model.layers)):
            self.example["layer%d_state" % i] = {}
        self._capture()

    # -- weight-only quantities, once per get_samples call -------------------------------
    def refresh(self):
        pol, h1, A = self.pol, self.h1, self.A
        with torch.no_grad():
            dst = [w for w in self.lwT] + [self.fcT[:, :h1], self.fc_b[:h1], self.outT[:h1, :A], self.out_b[:A]]
            src = [lin.weight.t() for lin in self.leading] + [self.fc.weight.t(), self.fc.bias, pol.out_layer.weight.t(), pol.out_layer.bias]
            if self.dueling:
                dst += [self.fcT[:, h1:], self.fc_b[h1:], self.outT[h1:, A:], self.out_b[A:]]
                src += [pol.value_hidden_layer.weight.t(), pol.value_hidden_layer.bias, pol.value_layer.weight.t(), pol.value_layer.bias]
            if self.iqn:
                dst.append(self.wqT)
                src.append(pol.quantile_layer.weight.t())
            for d, s in zip(dst, src):
                d.copy_(s.detach())

    # -- pieces ------------------------------------------------------------------------------
    def _conv1(self, obs, packed=False):
        """No input layer: an observation that is not the static input block already is staged into it."""
        if obs.data_ptr() != self.x_in.data_ptr():
            self.x_in.copy_(obs.reshape(self.E, self.O))

    def _body(self):
        """The whole network and the selection: reads x_in, writes actions, qvalues."""
        pol = self.pol
        greedy = self.expo is None
        taus = None
        if self.iqn and not self.in_kernel_taus:
            self.taus.copy_(pol._draw_taus(self.E * self.N))     # a test's tau_source replaces the draw
            taus = self.taus
        lead = self.leading
        quant = self.iqn
        check(lib.mirl_act_mlp_fwd(
            *self.shape, self.h1, 1 if self.need_q else 0, ptr(self.x_in),
            ptr(self.lwT[0]) if len(lead) >= 1 else None, ptr(lead[0].bias) if len(lead) >= 1 else None,
            ptr(self.lwT[1]) if len(lead) >= 2 else None, ptr(lead[1].bias) if len(lead) >= 2 else None,
            ptr(self.freq) if quant else None, ptr(taus), ptr(self.wqT) if quant else None,
            ptr(pol.quantile_layer.bias) if quant else None, ptr(self.fcT), ptr(self.fc_b), ptr(self.outT), ptr(self.out_b),
            None if greedy else ptr(self.eps), None if greedy else ptr(self.expo), self.eps_min, self.rng_seed, ptr(self.rng_step),
            ptr(self.actions), ptr(self.qvalues), None, stream()), "mirl_act_mlp_fwd")


class FastMlpAcStep(FastMlpStep):
    """The same step for an actor-critic (A2C / PPO) MLP policy under a Categorical head (cartpole_ppo / cartpole_a2c:
    4 -> 64 -> 64 -> [2 logits | value]), opt-in through acting.extra_args.fused_step (Actor(fused_actor_critic=True)).

    The one launch is mirl_act_mlp_ac_fwd (csrc/act_mlp.hip k_act_mlp<true>): the leading layers, the last FC, ONE product
    [logits | value] over outT = [logits_layer.weight; critic.weight]^T, and on that row the sampling head of
    k_actor_head_ac_rng with its Philox draw — the block where the Q-learning step keeps its q-values is [E, 2] =
    [log-probability | value], and the sink is the on-policy history (history/online_device.py: one mirl_online_append per
    vector step, the float32 observation handed over as its bytes).  Per vector step: env step, mirl_actor_pre, the append,
    the network — four launches, four nodes per step of a captured rollout.  The pre-step, the sink protocol, the rollout
    capture, the MIRL_ROLLOUT_* switches and the Philox keying are inherited unchanged."""
    AC = True

    @staticmethod
    def _mlp_parts(pol):
        """-> (leading Linears, the last FC's Linear, False), else a string that says what is in the way."""
        parts = FastMlpStep._fc_stack(pol)
        if isinstance(parts, str):
            return parts
        last = parts[-1]
        logits, critic = pol.actor.logits_layer, pol.critic
        if logits.in_features != last.out_features or critic.in_features != last.out_features or critic.out_features != 1:
            return "the logits layer and the critic do not both read the last FC module"
        if logits.bias is None or critic.bias is None:
            return "the logits layer or the critic has no bias"
        return parts[:-1], last, False

    @staticmethod
    def _shape(pol, parts, E, A):
        """FastMlpStep._shape's tuple with N = 1, D = 0, NO = A + 1: (E, O, L, widths, 1, 0, HID, A + 1, A)."""
        leading, last, _ = parts
        O = leading[0].in_features if leading else last.in_features
        widths = (C.c_int32 * 2)(*([lin.out_features for lin in leading] + [0, 0])[:2])
        return (E, O, len(leading), widths, 1, 0, last.out_features, A + 1, A)

    @staticmethod
    def _ac_args(shape):
        """The arguments of mirl_act_mlp_ac_supported: (E, O, L, widths, HID, A)."""
        return shape[:4] + (shape[6], shape[8])

    @staticmethod
    def why_not(actor, pol=None):
        """None when the step covers this actor's policy and env, else the reason as a string."""
        pol = pol if pol is not None else actor._policy
        try:
            if not hasattr(pol, "actor_head_ac_raw"):
                return "the policy is not an actor-critic policy"
            if not hasattr(actor._action_space, "n") or pol.has_normal_head():
                return "the action space is not Discrete"
            if pol.why_not_on_device() is not None:
                return pol.why_not_on_device()
            if not getattr(pol, "is_cuda", lambda: False)():
                return "the policy is not on the GPU"
            parts = FastMlpAcStep._mlp_parts(pol)
            if isinstance(parts, str):
                return parts
            if pol.model.layer_pre_processors:
                return "the model has layer pre-processors"
            space = actor._vec_env.observation_space
            if hasattr(space, "spaces") or str(getattr(space, "dtype", "")) != "float32" or len(tuple(space.shape)) != 1:
                return "the observation space is not a float32 vector"
            if not hasattr(actor._vec_env, "step_device"):
                return "the env does not step on the device"
            shape = FastMlpAcStep._shape(pol, parts, actor._num_envs, actor._action_space.n)
            if shape[1] != int(space.shape[0]):
                return "the first layer does not read the observation"
            if pol.actor.logits_layer.out_features != shape[8]:
                return "the logits layer does not have one output per action"
            if not lib.mirl_act_mlp_ac_supported(*FastMlpAcStep._ac_args(shape)):
                return "mirl_act_mlp_ac_supported refuses the shape (E, O, L, widths, HID, A) = %r" % (
                    shape[:3] + (list(shape[3])[:shape[2]], shape[6], shape[8]),)
            return None
        except Exception as e:                           # a policy this code does not know: not covered
            return "%s: %s" % (type(e).__name__, e)

    @staticmethod
    def supports(actor):
        return FastMlpAcStep.why_not(actor) is None

    def set_need_q(self, need_q):
        pass                                             # the [log-probability | value] pair is always evaluated

    def refresh(self):
        pol, A = self.pol, self.A
        with torch.no_grad():
            dst = [w for w in self.lwT] + [self.fcT, self.fc_b, self.outT[:, :A], self.outT[:, A:], self.out_b[:A], self.out_b[A:]]
            src = [lin.weight.t() for lin in self.leading] + [self.fc.weight.t(), self.fc.bias, pol.actor.logits_layer.weight.t(),
                                                              pol.critic.weight.t(), pol.actor.logits_layer.bias, pol.critic.bias]
            for d, s in zip(dst, src):
                d.copy_(s.detach())

    def _body(self):
        """The whole network and the sampling head: reads x_in, writes actions and the [log-probability | value] block."""
        lead = self.leading
        remap = self.expo is not None                    # the evaluator's fixed epsilon; training passes none
        check(lib.mirl_act_mlp_ac_fwd(
            *self._ac_args(self.shape), ptr(self.x_in),
            ptr(self.lwT[0]) if len(lead) >= 1 else None, ptr(lead[0].bias) if len(lead) >= 1 else None,
            ptr(self.lwT[1]) if len(lead) >= 2 else None, ptr(lead[1].bias) if len(lead) >= 2 else None,
            ptr(self.fcT), ptr(self.fc_b), ptr(self.outT), ptr(self.out_b),
            ptr(self.eps) if remap else None, ptr(self.expo) if remap else None, self.eps_min, self.rng_seed, ptr(self.rng_step),
            0, ptr(self.actions), ptr(self.qvalues), 2, None, stream()), "mirl_act_mlp_ac_fwd")
