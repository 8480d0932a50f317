"""The actor-critic form of the fused MLP acting kernel (csrc/act_mlp.hip k_act_mlp<true>, mirl_act_mlp_ac_fwd) restated: the
test shapes with their seeded operands, the layers in torch at a chosen precision, the sampling head on the Philox uniform
(tests/actor_critic_restate.head on tests/pointwise_restate's Philox), the evaluation's epsilon remap on words 2 and 3 of the
same block in NumPy, and the launches through the C-ABI.  Reference order: rltime/policies/torch/actor_critic.py:37-71,
eval.py:124-131.  Used by tests/test_fused_mlp_ac_cpu.py, tests/test_act_mlp_ac_gpu.py and tests/test_fused_mlp_ac_step_gpu.py."""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import actor_critic_restate as AR
from tests import pointwise_restate as PR

# (E, O, leading widths, HID, A): the smallest shapes that reach each branch of dense_rb<1> and of the head
SHAPES = {
    "shipped": (16, 4, [64], 64, 2),                    # cartpole_ppo
    "no-leading-layer": (5, 5, [], 40, 3),              # L = 0, J < 64, a 20-byte observation
    "wide": (3, 64, [256, 200], 512, 31),               # two passes over J, K > one tile, J not a multiple of 64
    "limit": (2, 64, [256, 256], 512, 32),              # NO = 33
    "one-action": (4, 4, [64], 64, 1),                  # S = 1, logp = 0
}
SEEDS = {"shipped": 11, "no-leading-layer": 12, "wide": 13, "limit": 14, "one-action": 15}
# the key of the kernel tests' draws and the two step words they run at (the second one has a high word)
RNG_SEED, STEPS = 0x5EED0AC, (5, 2 ** 32 + 7)
MLP = {"type": "sequential", "args": {"layer_configs": [{"type": "fc", "args": {"fc_size": 64}}, {"type": "fc", "args": {"fc_size": 64}}]}}


class Case:
    """The operands of one launch, on the CPU, in the layouts the policy holds them: Linear weights (out, in); wout is
    [logits_layer.weight; critic.weight], (A + 1, HID), dense."""

    def __init__(self, name):
        self.name = name
        self.E, self.O, self.widths, self.HID, self.A = SHAPES[name]
        self.W = self.widths[-1] if self.widths else self.O
        self.NO = self.A + 1
        g = torch.Generator().manual_seed(SEEDS[name])
        rn = lambda *s: torch.randn(*s, generator=g)           # noqa: E731
        self.obs = rn(self.E, self.O) * 0.7
        self.leading, k = [], self.O
        for w in self.widths:
            self.leading.append((rn(w, k) / math.sqrt(k), rn(w) * 0.1))
            k = w
        self.wfc, self.bfc = rn(self.HID, self.W) / math.sqrt(self.W), rn(self.HID) * 0.1
        self.wout, self.bout = rn(self.NO, self.HID) / math.sqrt(self.HID), rn(self.NO) * 0.1

    def widths_arg(self):
        return (C.c_int32 * 2)(*(list(self.widths) + [0, 0])[:2])

    def ac_shape_args(self):
        """(E, O, L, widths, HID, A) as mirl_act_mlp_ac_supported takes them."""
        return (self.E, self.O, len(self.widths), self.widths_arg(), self.HID, self.A)

    def q_shape_args(self):
        """The same network to mirl_act_mlp_fwd: a plain head of A + 1 "actions", N = 1, D = 0."""
        return (self.E, self.O, len(self.widths), self.widths_arg(), 1, 0, self.HID, self.NO, self.NO)


def reference(case, dtype, device="cpu"):
    """-> the product row [logits | value], (E, A + 1), at `dtype` on `device`."""
    c = case
    to = lambda t: t.to(device=device, dtype=dtype)             # noqa: E731
    f = to(c.obs)
    for w, b in c.leading:
        f = F.relu(F.linear(f, to(w), to(b)))
    hid = F.relu(F.linear(f, to(c.wfc), to(c.bfc)))
    return F.linear(hid, to(c.wout), to(c.bout))


# ---- the head and the remap on the step's Philox block ------------------------------------------------------------------------------
def philox_words(seed, step, E):
    """(E, 4) uint64: the block philox_4x32(seed, step, e) of every env."""
    return np.array([PR.philox_4x32(seed, step, e) for e in range(E)], dtype=np.uint64)


def uniform24(words):
    """float32(word >> 8) * 2^-24, exact in float32."""
    return ((words >> np.uint64(8)).astype(np.float64) / 16777216.0).astype(np.float32)


def head(rows, seed, step, greedy=False):
    """rows (E, A + 1) float32 [logits | value] -> (actions (E,), log-probabilities (E,) float64, values (E,) float32): the
    sampling head on u = uniform24(word 0), or the first maximum."""
    rows = np.asarray(rows, dtype=np.float32)
    E, A = rows.shape[0], rows.shape[1] - 1
    u = None if greedy else uniform24(philox_words(seed, step, E)[:, 0])
    actions, logp = AR.head(rows[:, :A].astype(np.float64), u, greedy=greedy)
    return actions, logp, rows[:, A].copy()


def eps_remap(actions, seed, step, A, eps, expo=None, eps_min=0.0):
    """The evaluation's remap: per = float32(max(eps ** expo_e, eps_min)) (float64 pow), uf = uniform24(word 2), and where
    uf < per the action becomes (word 3 * A) >> 32.  -> (actions (E,), rows within one float32 ulp of uf = per (E,) bool)."""
    actions = np.asarray(actions)
    E = len(actions)
    words = philox_words(seed, step, E)
    ex = np.ones(E) if expo is None else np.asarray(expo, dtype=np.float64)
    per = np.maximum(np.power(np.full(E, float(eps)), ex), float(eps_min)).astype(np.float32)
    uf = uniform24(words[:, 2])
    rnd = ((words[:, 3] * np.uint64(A)) >> np.uint64(32)).astype(np.int64)
    near = np.abs(uf.astype(np.float64) - per.astype(np.float64)) <= np.spacing(per).astype(np.float64)
    return np.where(uf < per, rnd, actions.astype(np.int64)), near


# ---- the launches ---------------------------------------------------------------------------------------------------------------------
def _p(x):
    return C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p(None)


class DeviceCase:
    """The case's operands on the GPU in the kernel's layouts: every weight transposed, [K][J] row-major."""

    def __init__(self, case, device="cuda"):
        c = self.case = case
        d = lambda t: t.to(device).contiguous()                 # noqa: E731
        t = lambda w: w.t().contiguous().to(device)             # noqa: E731
        self.obs = d(c.obs)
        self.lwT = [t(w) for w, _ in c.leading] + [None, None]
        self.lb = [d(b) for _, b in c.leading] + [None, None]
        self.fcT, self.fcb, self.outT, self.outb = t(c.wfc), d(c.bfc), t(c.wout), d(c.bout)
        self.device = device

    def args(self, seed, step, greedy=0, eps=None, expo=None, eps_min=0.0, actions=None, policy=None, out_pitch=2,
             logits_out="own"):
        """The argument list of mirl_act_mlp_ac_fwd and the output tensors (actions, policy, logits_out)."""
        c = self.case
        self.step = torch.tensor([step], dtype=torch.int64, device=self.device)
        self.eps = torch.tensor(eps, dtype=torch.float64, device=self.device) if eps is not None else None
        actions = torch.full((c.E,), -1, dtype=torch.int32, device=self.device) if actions is None else actions
        policy = torch.full((c.E, out_pitch), float("nan"), device=self.device) if policy is None else policy
        if isinstance(logits_out, str):
            logits_out = torch.full((c.E, c.NO), float("nan"), device=self.device)
        a = [*c.ac_shape_args(), _p(self.obs), _p(self.lwT[0]), _p(self.lb[0]), _p(self.lwT[1]), _p(self.lb[1]), _p(self.fcT),
             _p(self.fcb), _p(self.outT), _p(self.outb), _p(self.eps), _p(expo), float(eps_min), seed, _p(self.step), greedy,
             _p(actions), _p(policy), out_pitch, _p(logits_out), C.c_void_p(torch.cuda.current_stream().cuda_stream)]
        return a, (actions, policy, logits_out)

    def launch(self, seed=RNG_SEED, step=STEPS[0], **kw):
        """One mirl_act_mlp_ac_fwd launch -> (actions int32 [E], policy [E][out_pitch], logits_out [E][A + 1] or None)."""
        from rltime_amd._lib import lib, check
        a, outs = self.args(seed, step, **kw)
        check(lib.mirl_act_mlp_ac_fwd(*a), "mirl_act_mlp_ac_fwd")
        return outs

    def launch_q(self):
        """The same weights through mirl_act_mlp_fwd as a plain, non-dueling head of A + 1 "actions" (N = 1, D = 0,
        need_q = 1) -> its q-values [E][A + 1]: the output rows themselves (the mean over one row divides by 1)."""
        from rltime_amd._lib import lib, check
        c = self.case
        step = torch.tensor([0], dtype=torch.int64, device=self.device)
        actions = torch.full((c.E,), -1, dtype=torch.int32, device=self.device)
        q = torch.full((c.E, c.NO), float("nan"), device=self.device)
        check(lib.mirl_act_mlp_fwd(
            *c.q_shape_args(), c.HID, 1, _p(self.obs), _p(self.lwT[0]), _p(self.lb[0]), _p(self.lwT[1]), _p(self.lb[1]),
            None, None, None, None, _p(self.fcT), _p(self.fcb), _p(self.outT), _p(self.outb), None, None, 0.0, 0, _p(step),
            _p(actions), _p(q), None, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mirl_act_mlp_fwd")
        return q


# ---- the step test's CartPole rollout on the CPU ------------------------------------------------------------------------------------
STEP_E, STEP_ENV_SEED, STEP_POLICY_SEED, STEP_RNG_SEED = 16, 5, 0, 0xAC5EED
FIRST_WORD = 1                     # the step word the action of vector step 0 is drawn at (the constructor's pre-step moved it to 1)


def step_policy(env, cuda):
    """The policy of the step test: cartpole_ppo's model under torch seed STEP_POLICY_SEED (built on the CPU, then moved)."""
    from rltime_amd.policies.actor_critic import ActorCriticPolicy
    torch.manual_seed(STEP_POLICY_SEED)
    return ActorCriticPolicy.create(model_config=MLP, observation_space=env.observation_space, action_space=env.action_space,
                                    cuda=cuda)


def change_weights(pol):
    """The step test's "learner update" after vector step 4 (tests/test_fused_actor_critic_gpu.py's)."""
    with torch.no_grad():
        pol.actor.logits_layer.weight.mul_(4.0)
        pol.critic.bias.add_(0.5)


def input_tree(obs):
    return {"x": obs, "layer0_state": {}, "layer1_state": {}}
