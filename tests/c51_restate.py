"""CPU restatement of the C51 (distributional DQN) arithmetic the reference runs in
rltime/training/torch/dist_dqn.py — the target projection (:30-97) and the loss with its
gradient (:99-142) — in plain torch on the CPU, written from the formulas, for the tests
and the fixture generator (tests/golden/generate_dist_dqn.py asserts it reproduces the
reference bit for bit).

Projection "reference": Tz_j = (r + mask * gamma^n) * z_j, clamped; b = (Tz - vmin) / dz;
bin floor(b) gets p_j (ceil(b) - b), bin ceil(b) gets p_j (b - floor(b)), all lower
shares first (ascending j), then all upper shares.  An atom whose b is an integer
contributes nothing.  Projection "paper": Tz_j = r + mask * gamma^n * z_j and such an atom
keeps its whole mass."""
import torch
import torch.nn.functional as F


def select_actions(logits_select, support):
    """argmax_a sum_j softmax(logits)_aj z_j (first maximum)."""
    return (F.softmax(logits_select, dim=-1) * support).sum(2).argmax(dim=-1)


def project(p, returns, nsteps, masks, support, gamma, vmin, vmax, projection="reference"):
    """p (M, Z) of the selected action -> (M, Z) projected target.  Arithmetic in p's dtype."""
    M, Z = p.shape
    dt = p.dtype
    r, n, mk = (torch.as_tensor(x).to(dt).reshape(M, 1) for x in (returns, nsteps, masks))
    z = support.to(dt)
    disc = mk * (gamma ** n)
    tz = (r + disc) * z if projection == "reference" else r + disc * z
    tz = tz.clamp(min=vmin, max=vmax)
    b = (tz - vmin) / (float(vmax - vmin) / (Z - 1))
    lo, up = b.floor(), b.ceil()
    lo_share = p * (up - b)
    if projection == "paper":
        lo_share = torch.where(lo == up, p, lo_share)
    out = torch.zeros(M * Z, dtype=dt)
    offset = (torch.arange(M) * Z).unsqueeze(1)
    out.index_add_(0, (lo.long() + offset).reshape(-1), lo_share.reshape(-1))
    out.index_add_(0, (up.long() + offset).reshape(-1), (p * (b - lo)).reshape(-1))
    return out.view(M, Z)


def target(logits_target, logits_select, support, returns, nsteps, masks, gamma, vmin, vmax, projection="reference"):
    best = select_actions(logits_select, support)
    p = F.softmax(logits_target[torch.arange(logits_target.shape[0]), best], dim=-1)
    return project(p, returns, nsteps, masks, support, gamma, vmin, vmax, projection)


def row_losses(logits, actions, targets, mode="crossentropy", kappa=1.0):
    """-> per-row loss (M,) of the chosen action's softmax against the target distribution."""
    p = F.softmax(logits[torch.arange(logits.shape[0]), torch.as_tensor(actions).long()], dim=-1)
    if mode == "crossentropy":
        return -(targets * p.clamp(1e-5, 1 - 1e-5).log()).sum(1)
    e = p - targets
    if mode == "mse":
        return e.pow(2).sum(1)
    a = e.abs()
    return torch.where(a <= kappa, 0.5 * e.pow(2), kappa * (a - 0.5 * kappa)).sum(1)


def loss(logits, actions, targets, weights=None, mode="crossentropy", kappa=1.0, timesteps=1,
         batch_mode="mean", time_mode=None):
    """-> (aggregated scalar loss, unweighted row losses)."""
    rows = row_losses(logits, actions, targets, mode, kappa)
    agg = rows if weights is None else rows * torch.as_tensor(weights).to(rows.dtype)
    red = {"mean": torch.mean, "sum": torch.sum}
    if time_mode:
        agg = red[time_mode](agg.view(timesteps, -1), dim=0)
    return red[batch_mode](agg), rows
