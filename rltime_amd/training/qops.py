"""Fused Q-learning target / loss ops (librltime_hip qmath kernels) as torch
functions.  No torch fallback: inputs must be CUDA tensors.

Reference arithmetic restated by the kernels:
  torch_trainer.py:46-78,124-147   value rescaling + n-step bootstrap target
  training/torch/dqn.py:52-71      DQN / double-Q bootstrap value
  training/torch/iqn.py:36-52      IQN bootstrap value
  training/torch/dqn.py:98-130,141-161   DQN loss, IS weights, aggregation
  training/torch/iqn.py:77-120     IQN pairwise quantile-Huber loss
  training/torch/dist_dqn.py:30-97,99-142   C51 target projection and loss (csrc/c51.hip)
"""
import torch

from .._lib import lib, check, ptr, stream


def _f32(t):
    assert t.is_cuda, "rltime_amd.qops needs CUDA tensors (no CPU fallback)"
    return t.detach().to(torch.float32).contiguous()


def row_scale(rows, timesteps, batch_mode="mean", time_mode=None):
    """d(loss)/d(row loss) of dqn.py:120-130 (_aggregate_losses): every
    combination of mean/sum over time then batch is one constant factor."""
    s = 1.0
    count = rows
    if time_mode:
        if time_mode == "mean":
            s /= timesteps
        count = rows // timesteps
    if batch_mode == "mean":
        s /= count
    return s


def q_target_dqn(q_target, q_select, returns, nsteps, masks, gamma, vf_eps=None):
    q_target, q_select = _f32(q_target), _f32(q_select)
    M, A = q_target.shape
    out = torch.empty(M, dtype=torch.float32, device=q_target.device)
    check(lib.mirl_q_target_dqn(
        M, A, ptr(q_target), ptr(q_select), ptr(_f32(returns)), ptr(_f32(nsteps)),
        ptr(_f32(masks)), float(gamma), float(vf_eps or 0.0), ptr(out), stream()),
        "mirl_q_target_dqn")
    return out


def q_target_iqn(z_target, z_select, returns, nsteps, masks, gamma, vf_eps=None):
    z_target, z_select = _f32(z_target), _f32(z_select)
    M, Nt, A = z_target.shape
    Ns = z_select.shape[1]
    out = torch.empty((M, Nt), dtype=torch.float32, device=z_target.device)
    check(lib.mirl_q_target_iqn(
        M, Nt, Ns, A, ptr(z_target), ptr(z_select), ptr(_f32(returns)),
        ptr(_f32(nsteps)), ptr(_f32(masks)), float(gamma), float(vf_eps or 0.0),
        ptr(out), stream()), "mirl_q_target_iqn")
    return out


_PROJECTIONS = {"reference": 0, "paper": 1}
_C51_MODES = {"crossentropy": 0, "mse": 1, "huber": 2}


def q_target_c51(logits_target, logits_select, support, returns, nsteps, masks, gamma, vmin, vmax,
                 projection="reference"):
    """dist_dqn.py:30-97 -> (M, Z) target distributions.  logits_* (M, A, Z); logits_select may be
    logits_target itself (no double-Q).  projection="paper" is not the reference's formula (see
    include/mirl.h mirl_q_target_c51)."""
    same = logits_select is logits_target
    logits_target = _f32(logits_target)
    logits_select = logits_target if same else _f32(logits_select)
    M, A, Z = logits_target.shape
    assert logits_select.shape == (M, A, Z)
    support = _f32(support)
    assert support.shape == (Z,)
    out = torch.empty((M, Z), dtype=torch.float32, device=logits_target.device)
    delta_z = float(vmax - vmin) / (Z - 1)          # dist_dqn.py:81, a Python float like the reference's
    check(lib.mirl_q_target_c51(
        M, A, Z, ptr(logits_target), ptr(logits_select), ptr(support), ptr(_f32(returns)), ptr(_f32(nsteps)),
        ptr(_f32(masks)), float(gamma), float(vmin), float(vmax), delta_z, _PROJECTIONS[projection], ptr(out),
        stream()), "mirl_q_target_c51")
    return out


class _C51Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, actions, targets, weights, mode, kappa, scale):
        xc = _f32(logits)
        M, A, Z = xc.shape
        rows = torch.empty(M, dtype=torch.float32, device=xc.device)
        rep = torch.empty(M, dtype=torch.float32, device=xc.device)
        dx = torch.empty_like(xc)
        w = _f32(weights) if weights is not None else None
        check(lib.mirl_loss_c51(
            M, A, Z, ptr(xc), ptr(actions.to(torch.int64).contiguous()), ptr(_f32(targets)), ptr(w),
            _C51_MODES[mode], float(kappa), float(scale), ptr(rows), ptr(dx), ptr(rep), stream()), "mirl_loss_c51")
        ctx.save_for_backward(dx)
        ctx.mark_non_differentiable(rep)
        return rows.sum() * scale, rep

    @staticmethod
    def backward(ctx, g_loss, g_rep):
        (dx,) = ctx.saved_tensors
        return dx * g_loss, None, None, None, None, None, None


class _DQNLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, actions, targets, weights, kappa, mode, scale):
        qc = _f32(q)
        M, A = qc.shape
        rows = torch.empty(M, dtype=torch.float32, device=qc.device)
        td = torch.empty(M, dtype=torch.float32, device=qc.device)
        dq = torch.empty_like(qc)
        w = _f32(weights) if weights is not None else None
        check(lib.mirl_loss_dqn(
            M, A, ptr(qc), ptr(actions.to(torch.int64).contiguous()), ptr(_f32(targets)),
            ptr(w), float(kappa), 1 if mode == "mse" else 0, float(scale),
            ptr(rows), ptr(dq), ptr(td), stream()), "mirl_loss_dqn")
        ctx.save_for_backward(dq)
        ctx.mark_non_differentiable(td)
        return rows.sum() * scale, td

    @staticmethod
    def backward(ctx, g_loss, g_td):
        (dq,) = ctx.saved_tensors
        return dq * g_loss, None, None, None, None, None, None


class _IQNLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, taus, actions, targets, weights, kappa, scale):
        zc = _f32(z)
        M, N, A = zc.shape
        Nt = targets.shape[1]
        rows = torch.empty(M, dtype=torch.float32, device=zc.device)
        rep = torch.empty(M, dtype=torch.float32, device=zc.device)
        dz = torch.empty_like(zc)
        w = _f32(weights) if weights is not None else None
        check(lib.mirl_loss_iqn(
            M, N, Nt, A, ptr(zc), ptr(_f32(taus).reshape(M, N)),
            ptr(actions.to(torch.int64).contiguous()), ptr(_f32(targets)), ptr(w),
            float(kappa), float(scale), ptr(rows), ptr(dz), ptr(rep), stream()),
            "mirl_loss_iqn")
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(rep)
        return rows.sum() * scale, rep

    @staticmethod
    def backward(ctx, g_loss, g_rep):
        (dz,) = ctx.saved_tensors
        return dz * g_loss, None, None, None, None, None, None


def dqn_loss(q, actions, targets, weights=None, kappa=1.0, mode="huber",
             timesteps=1, batch_mode="mean", time_mode=None):
    """-> (scalar loss differentiable w.r.t. q, signed td report (M,))."""
    scale = row_scale(q.shape[0], timesteps, batch_mode, time_mode)
    return _DQNLoss.apply(q, actions, targets, weights, kappa, mode, scale)


def iqn_loss(z, taus, actions, targets, weights=None, kappa=1.0,
             timesteps=1, batch_mode="mean", time_mode=None):
    """-> (scalar loss differentiable w.r.t. z, mean |td| report (M,))."""
    scale = row_scale(z.shape[0], timesteps, batch_mode, time_mode)
    return _IQNLoss.apply(z, taus, actions, targets, weights, kappa, scale)


def c51_loss(logits, actions, targets, weights=None, mode="crossentropy", kappa=1.0,
             timesteps=1, batch_mode="mean", time_mode=None):
    """dist_dqn.py:99-142 -> (scalar loss differentiable w.r.t. logits (M, A, Z), unweighted row loss report (M,))."""
    scale = row_scale(logits.shape[0], timesteps, batch_mode, time_mode)
    return _C51Loss.apply(logits, actions, targets, weights, mode, kappa, scale)


class _ACLoss(torch.autograd.Function):
    """csrc/actor_critic.hip mirl_ac_loss: the loss scalar is stats[0]; its gradients come out of the same launch."""

    @staticmethod
    def forward(ctx, logits, values, actions, targets, acting_values, old_log_probs, vf_coef, entropy_factor, clip_value,
                adv_norm):
        z, v = _f32(logits), _f32(values)
        M, A = z.shape
        dz, dv = torch.empty_like(z), torch.empty_like(v)
        stats = torch.empty(5, dtype=torch.float32, device=z.device)
        old = _f32(old_log_probs) if old_log_probs is not None else None
        check(lib.mirl_ac_loss(
            M, A, ptr(z), z.stride(0), ptr(v), ptr(actions.detach().to(torch.int32).contiguous()), ptr(_f32(targets)),
            ptr(_f32(acting_values)), ptr(old), float(vf_coef), float(entropy_factor),
            float(clip_value if clip_value is not None else 0.0), 1 if adv_norm else 0, ptr(dz), A, ptr(dv), None,
            ptr(stats), stream()), "mirl_ac_loss")
        ctx.save_for_backward(dz, dv)
        ctx.mark_non_differentiable(stats)
        return stats[0].clone(), stats

    @staticmethod
    def backward(ctx, g_loss, g_stats):
        dz, dv = ctx.saved_tensors
        return dz * g_loss, dv * g_loss, None, None, None, None, None, None, None, None


class _ACLossNormal(torch.autograd.Function):
    """csrc/actor_critic.hip mirl_ac_loss_normal: the loss scalar is stats[0]; its three gradients come out of the same launch."""

    @staticmethod
    def forward(ctx, mean, logstd, values, actions, targets, acting_values, old_log_probs, vf_coef, entropy_factor, clip_value,
                adv_norm):
        m, ls, v = _f32(mean), _f32(logstd), _f32(values)
        M, D = m.shape
        act = _f32(actions.detach()).reshape(M, -1)
        if act.shape[1] != D or ls.numel() != D:
            raise ValueError("ac_loss_normal: mean (M, D), logstd (D,), actions (M, D); got %s, %s, %s"
                             % (tuple(m.shape), tuple(ls.shape), tuple(actions.shape)))
        dm, dls, dv = torch.empty_like(m), torch.empty_like(ls), torch.empty_like(v)
        stats = torch.empty(5, dtype=torch.float32, device=m.device)
        old = _f32(old_log_probs) if old_log_probs is not None else None
        check(lib.mirl_ac_loss_normal(
            M, D, ptr(m), m.stride(0), ptr(ls), ptr(v), ptr(act), ptr(_f32(targets)), ptr(_f32(acting_values)), ptr(old),
            float(vf_coef), float(entropy_factor), float(clip_value if clip_value is not None else 0.0), 1 if adv_norm else 0,
            ptr(dm), D, ptr(dls), ptr(dv), None, ptr(stats), stream()), "mirl_ac_loss_normal")
        ctx.save_for_backward(dm, dls, dv)
        ctx.mark_non_differentiable(stats)
        return stats[0].clone(), stats

    @staticmethod
    def backward(ctx, g_loss, g_stats):
        dm, dls, dv = ctx.saved_tensors
        return dm * g_loss, dls * g_loss, dv * g_loss, None, None, None, None, None, None, None, None


def ac_loss_normal(mean, logstd, values, actions, targets, acting_values, old_log_probs=None, vf_coef=1.0, entropy_factor=0.0,
                   clip_value=None, adv_norm=False):
    """ac_loss under the Normal head (distributions/normal.py): mean (M, D), logstd (D,), float32 actions (M, D) -> (scalar
    loss differentiable w.r.t. mean, logstd and values, stats (5,)); the entropy is the mean over the components."""
    return _ACLossNormal.apply(mean, logstd, values, actions, targets, acting_values, old_log_probs, vf_coef, entropy_factor,
                               clip_value, adv_norm)


def ac_loss(logits, values, actions, targets, acting_values, old_log_probs=None, vf_coef=1.0, entropy_factor=0.0,
            clip_value=None, adv_norm=False):
    """training/torch/a2c.py:101-141 with the gain of a2c.py:90-99 (old_log_probs None) or ppo.py:39-56, forward and
    backward in one launch -> (scalar loss differentiable w.r.t. logits (M, A) and values (M,), stats (5,) = loss,
    value loss, policy loss, mean entropy, mean value)."""
    return _ACLoss.apply(logits, values, actions, targets, acting_values, old_log_probs, vf_coef, entropy_factor,
                         clip_value, adv_norm)
