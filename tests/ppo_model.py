"""fp64 model of the clipped-surrogate (PPO) loss of sample reuse, the reference of unreal_ppo_heads_loss_grad.

Per active row, with base_loss_grad's conventions (probabilities clipped to [1e-20, 1]; `un` = 1 where the clip passes the
gradient): pc' = clip(pi'[a]), p_old = clip(pi_old[a]), rho = pc' / p_old,
    policy loss = -min(rho A, clip(rho, 1 - eps, 1 + eps) A) - beta H(pi'),   value loss = 0.25 (R - v')^2.
The unclipped term is the active one when rho A <= clip(rho) A (a tie counts as unclipped): d/dpc' = -A un / p_old, and 0
otherwise.  `ppo_loss` is the closed form in numpy; `surrogate_torch` the same loss as a differentiable torch expression
(the trainer tests back-propagate it through an fp64 trunk)."""
import numpy as np
import torch

P_LO = float(np.float32(1e-20))       # the kernels' lower clip bound is the fp32 constant
P_HI = 1.0


def ppo_loss(pi_new, v_new, pi_old, action, adv, R, active, eps, beta, scale):
    """pi_new [rows, A], v_new [rows], pi_old [rows, A] (or [rows]: the old probability of the action taken), action, adv, R,
    active [rows] -> dict: losses (policy, value, entropy; scaled), dlogits [rows, A], dv [rows] (scaled, 0 on inactive
    rows), clipped, counted, kl_sum = sum (rho - 1 - ln rho), abs_sum = sum |rho - 1|, and per row rho, unclipped."""
    p = np.asarray(pi_new, np.float64)
    rows, A = p.shape
    v = np.asarray(v_new, np.float64).reshape(rows)
    a = np.asarray(action).astype(np.int64).reshape(rows)
    adv = np.asarray(adv, np.float64).reshape(rows)
    R = np.asarray(R, np.float64).reshape(rows)
    on = np.asarray(active).reshape(rows) != 0
    po = np.asarray(pi_old, np.float64)
    po = po.reshape(rows, A)[np.arange(rows), a] if po.size == rows * A else po.reshape(rows)
    r = np.arange(rows)
    pc = np.clip(p, P_LO, P_HI)
    un = ((p >= P_LO) & (p <= P_HI)).astype(np.float64)
    lp = np.log(pc)
    H = -(p * lp).sum(1)
    p_old = np.clip(po, P_LO, P_HI)
    rho = pc[r, a] / p_old
    rc = np.clip(rho, 1.0 - eps, 1.0 + eps)
    s1, s2 = rho * adv, rc * adv
    unclipped = s1 <= s2
    g = beta * (lp + un)                                   # d/dpi of -beta H
    g[r, a] += np.where(unclipped, -adv * un[r, a] / p_old, 0.0)
    dot = (p * g).sum(1, keepdims=True)
    dlogits = scale * p * (g - dot) * on[:, None]
    diff = R - v
    dv = scale * (-0.5 * diff) * on
    pl = -(np.minimum(s1, s2) + beta * H)
    losses = scale * np.array([pl[on].sum(), (0.25 * diff * diff)[on].sum(), H[on].sum()])
    return dict(losses=losses, dlogits=dlogits, dv=dv, clipped=int((~unclipped & on).sum()), counted=int(on.sum()),
                kl_sum=float((rho - 1.0 - np.log(rho))[on].sum()), abs_sum=float(np.abs(rho - 1.0)[on].sum()), rho=rho,
                unclipped=unclipped)


def surrogate_torch(pi, v, pi_old_a, a_onehot, adv, R, eps, beta):
    """The same loss over rows that are all active, differentiable in pi and v (fp64 tensors; pi_old_a [rows] is a
    constant) -> (policy_loss, value_loss, entropy [rows]) summed like oracle.model.base_loss."""
    pc = torch.clamp(pi, P_LO, P_HI)
    log_pi = torch.log(pc)
    entropy = -(pi * log_pi).sum(1)
    rho = (pc * a_onehot).sum(1) / torch.clamp(pi_old_a, P_LO, P_HI)
    s1, s2 = rho * adv, torch.clamp(rho, 1.0 - eps, 1.0 + eps) * adv
    surr = torch.where(s1 <= s2, s1, s2)                   # (a tie takes the unclipped term and its gradient)
    policy_loss = -(surr + entropy * beta).sum()
    value_loss = 0.25 * ((R - v) ** 2).sum()
    return policy_loss, value_loss, entropy


def edge_distance(rho, eps):
    """min over rows of the distance of rho to the nearer clip edge 1 - eps / 1 + eps."""
    rho = np.asarray(rho, np.float64)
    return float(np.minimum(np.abs(rho - (1.0 - eps)), np.abs(rho - (1.0 + eps))).min())
