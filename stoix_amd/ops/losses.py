"""RL loss functions (torch reference implementations).

Parity surface with /root/reference/stoix/utils/loss.py:
ppo_clip_loss :17-32, ppo_penalty_loss :35-47, dpo_loss :50-65,
clipped_value_loss :68-78, categorical_double_q_learning :81-103,
q_learning :106-124, double_q_learning :127-146, td_learning :149-163,
categorical_td_learning :166-187, munchausen_q_learning :190-223,
quantile_regression_loss / quantile_q_learning :226-314.

All are written against batched torch tensors; each is differentiable so the
update path can run under autograd (captured in a hip graph); the fused HIP
loss+grad kernels used by the Anakin fast path are numerics-tested against
these references (tests/test_losses.py).
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

Tensor = torch.Tensor


# ---------------------------------------------------------------- policy-side


def ppo_clip_loss(
    pi_log_prob_t: Tensor,
    b_pi_log_prob_t: Tensor,
    gae_t: Tensor,
    epsilon: float,
) -> Tensor:
    """PPO clipped surrogate (Schulman et al. 2017)."""
    ratio = torch.exp(pi_log_prob_t - b_pi_log_prob_t)
    loss1 = ratio * gae_t
    loss2 = torch.clamp(ratio, 1.0 - epsilon, 1.0 + epsilon) * gae_t
    return -torch.minimum(loss1, loss2).mean()


def ppo_penalty_loss(
    pi_log_prob_t: Tensor,
    b_pi_log_prob_t: Tensor,
    gae_t: Tensor,
    kl_penalty_coef: float,
) -> Tuple[Tensor, Tensor]:
    """PPO with KL penalty instead of clipping: ratio*A - beta*KL(b||pi)
    (reference loss.py:35-47). Returns (loss, mean_approx_kl)."""
    log_ratio = pi_log_prob_t - b_pi_log_prob_t
    ratio = torch.exp(log_ratio)
    # Unbiased low-variance KL(b||pi) estimator: (r - 1) - log r
    approx_kl = (ratio - 1.0) - log_ratio
    loss = -(ratio * gae_t - kl_penalty_coef * approx_kl).mean()
    return loss, approx_kl.mean()


def dpo_loss(
    pi_log_prob_t: Tensor,
    b_pi_log_prob_t: Tensor,
    gae_t: Tensor,
    alpha: float,
    beta: float,
) -> Tensor:
    """Drift (DPO) policy loss (reference loss.py:50-65; arXiv:2310.19102).

    drift+ = relu((r-1)A - alpha*tanh((r-1)A/alpha)) for A>=0,
    drift- = relu(log(r)A - beta*tanh(log(r)A/beta)) for A<0;
    loss = -(r*A - drift).
    """
    log_ratio = pi_log_prob_t - b_pi_log_prob_t
    ratio = torch.exp(log_ratio)
    is_pos = (gae_t >= 0.0).to(gae_t.dtype)
    r1a = (ratio - 1.0) * gae_t
    drift_pos = F.relu(r1a - alpha * torch.tanh(r1a / alpha))
    lra = log_ratio * gae_t
    drift_neg = F.relu(lra - beta * torch.tanh(lra / beta))
    drift = is_pos * drift_pos + (1.0 - is_pos) * drift_neg
    return -(ratio * gae_t - drift).mean()


def clipped_value_loss(
    pred_value_t: Tensor,
    behavior_value_t: Tensor,
    targets_t: Tensor,
    epsilon: float,
) -> Tensor:
    """Clipped value loss (reference loss.py:68-78): max of clipped and
    unclipped squared errors, 0.5 * mean."""
    clipped = behavior_value_t + torch.clamp(
        pred_value_t - behavior_value_t, -epsilon, epsilon
    )
    err = (pred_value_t - targets_t) ** 2
    err_clipped = (clipped - targets_t) ** 2
    return 0.5 * torch.maximum(err, err_clipped).mean()


# ----------------------------------------------------------------- value-side


def _huber(x: Tensor, delta: float) -> Tensor:
    if delta <= 0:
        return 0.5 * x**2
    abs_x = x.abs()
    return torch.where(abs_x <= delta, 0.5 * x**2, delta * (abs_x - 0.5 * delta))


def q_learning(
    q_tm1: Tensor,
    a_tm1: Tensor,
    r_t: Tensor,
    d_t: Tensor,
    q_t: Tensor,
    huber_loss_parameter: float = 0.0,
) -> Tensor:
    """1-step Q-learning loss (reference loss.py:106-124).

    target = r + d * max_a q_t;  loss = huber/mse(target - q_tm1[a]).
    ``d_t`` = gamma * (1 - done).
    """
    q_a = q_tm1.gather(-1, a_tm1.long().unsqueeze(-1)).squeeze(-1)
    target = (r_t + d_t * q_t.max(dim=-1).values).detach()
    return _huber(target - q_a, huber_loss_parameter).mean()


def double_q_learning(
    q_tm1: Tensor,
    q_t_value: Tensor,
    a_tm1: Tensor,
    r_t: Tensor,
    d_t: Tensor,
    q_t_selector: Tensor,
    huber_loss_parameter: float = 0.0,
) -> Tensor:
    """Double Q-learning (reference loss.py:127-146): action argmax from the
    online net (selector), value from the target net."""
    q_a = q_tm1.gather(-1, a_tm1.long().unsqueeze(-1)).squeeze(-1)
    best_a = q_t_selector.argmax(dim=-1, keepdim=True)
    q_target_a = q_t_value.gather(-1, best_a).squeeze(-1)
    target = (r_t + d_t * q_target_a).detach()
    return _huber(target - q_a, huber_loss_parameter).mean()


def td_learning(
    v_tm1: Tensor,
    r_t: Tensor,
    d_t: Tensor,
    v_t: Tensor,
    huber_loss_parameter: float = 0.0,
) -> Tensor:
    """1-step TD loss (reference loss.py:149-163)."""
    target = (r_t + d_t * v_t).detach()
    return _huber(target - v_tm1, huber_loss_parameter).mean()


def categorical_l2_project(
    z_p: Tensor,
    probs: Tensor,
    z_q: Tensor,
) -> Tensor:
    """Cramer projection of distribution (z_p, probs) onto support z_q
    (Bellemare et al. 2017; reference uses rlax.categorical_l2_project at
    loss.py:98,183). Batched: z_p [B, N], probs [B, N], z_q [M] -> [B, M]."""
    kq = z_q.shape[-1]
    vmin, vmax = z_q[0], z_q[-1]
    dz = (vmax - vmin) / (kq - 1)
    z_p = z_p.clamp(vmin, vmax)
    b = (z_p - vmin) / dz  # [B, N] fractional bin index
    lo = b.floor().clamp(0, kq - 1)
    hi = b.ceil().clamp(0, kq - 1)
    w_hi = b - lo
    w_lo = 1.0 - w_hi
    # when lo == hi (b integral), all weight to lo
    same = (lo == hi).to(probs.dtype)
    w_lo = w_lo + same * w_hi
    w_hi = w_hi * (1.0 - same)
    out = torch.zeros((*probs.shape[:-1], kq), dtype=probs.dtype, device=probs.device)
    out.scatter_add_(-1, lo.long(), probs * w_lo)
    out.scatter_add_(-1, hi.long(), probs * w_hi)
    return out


# ------------------------------------------------- fused C51 loss (c51.hip)

_C51_MAX_ATOMS = 1024
_C51_MAX_ACTIONS = 64


def c51_fused_enabled() -> bool:
    """STOIX_FUSED_C51=0 forces the torch composition (A/B timing)."""
    return os.environ.get("STOIX_FUSED_C51", "1") != "0"


def _single_support(atoms: Tensor) -> Optional[Tensor]:
    """The one support row behind ``atoms``: [N] as is, [B, N] only when it is
    an expanded view of one row (stride 0 on dim 0); else None."""
    if atoms.dim() == 1:
        return atoms
    if atoms.dim() == 2 and (atoms.shape[0] == 1 or atoms.stride(0) == 0):
        return atoms[0]
    return None


def _c51_kernel_eligible(q_logits_tm1: Tensor, q_logits_t: Tensor) -> bool:
    """The HIP path takes [B, A, atoms] fp32/bf16 logits on the GPU within
    the kernel's size limits."""
    for lg in (q_logits_tm1, q_logits_t):
        if not lg.is_cuda or lg.dtype not in (torch.float32, torch.bfloat16):
            return False
        if lg.dim() != 3 or not 1 <= lg.shape[2] <= _C51_MAX_ATOMS:
            return False
    return (
        q_logits_tm1.shape[:2] == q_logits_t.shape[:2]
        and 1 <= q_logits_tm1.shape[1] <= _C51_MAX_ACTIONS
    )


class _C51Loss(torch.autograd.Function):
    """Per-row C51 cross-entropy with its closed-form logits gradient.

    On the GPU forward and backward are the two c51.hip kernels; on the CPU
    they are the same math in torch (computed in the logits' dtype, so fp64
    checks the closed form). Nothing flows to r, d, the target logits, the
    selector or the atoms: the projected target is a constant.
    """

    @staticmethod
    def forward(ctx, logits_tm1, atoms_tm1, a_tm1, r_t, d_t, logits_t, atoms_t, selector):
        B, A, M = logits_tm1.shape
        if logits_tm1.is_cuda:
            from stoix_amd.ops import ext

            logits_tm1 = logits_tm1.contiguous()
            dev = logits_tm1.device
            empty = torch.empty(0, dtype=torch.float32, device=dev)
            ce = torch.empty(B, dtype=torch.float32, device=dev)
            lse = torch.empty(B, dtype=torch.float32, device=dev)
            target = torch.empty(B, M, dtype=torch.float32, device=dev)
            a_arg = empty.long() if a_tm1 is None else a_tm1.long()
            ext(required=True).c51_loss_fwd(
                logits_tm1,
                atoms_tm1.float().contiguous(),
                a_arg,
                r_t.float(),  # per-row vectors may be strided views
                d_t.float(),
                logits_t.contiguous(),
                atoms_t.float().contiguous(),
                empty if selector is None else selector.float().contiguous(),
                ce,
                lse,
                target,
            )
            ctx.save_for_backward(logits_tm1, a_arg, lse, target)
        else:
            cd = logits_tm1.dtype if logits_tm1.dtype == torch.float64 else torch.float32
            rows = torch.arange(B)
            best = selector.argmax(dim=-1) if selector is not None else torch.zeros(B, dtype=torch.long)
            p = F.softmax(logits_t.to(cd)[rows, best], dim=-1)  # [B, N]
            z_q = atoms_tm1.to(cd)
            vmin, vmax = z_q[0], z_q[-1]
            z = (r_t.to(cd).unsqueeze(-1) + d_t.to(cd).unsqueeze(-1) * atoms_t.to(cd)).clamp(vmin, vmax)
            bpos = (z - vmin) / ((vmax - vmin) / (M - 1)) if M > 1 else torch.zeros_like(z)
            lo = bpos.floor()
            w_hi = bpos - lo
            lo = lo.long().clamp(0, M - 1)
            hi = (lo + 1).clamp(max=M - 1)
            target = torch.zeros(B, M, dtype=cd)
            target.scatter_add_(-1, lo, p * (1.0 - w_hi))
            target.scatter_add_(-1, hi, p * w_hi)
            a_arg = torch.zeros(B, dtype=torch.long) if a_tm1 is None else a_tm1.long()
            a_ok = (a_arg >= 0) & (a_arg < A)
            logits_a = logits_tm1.to(cd)[rows, a_arg.clamp(0, A - 1)]  # [B, M]
            lse = torch.logsumexp(logits_a, dim=-1)
            ce = -(target * (logits_a - lse.unsqueeze(-1))).sum(-1)
            ce = torch.where(a_ok, ce, torch.full_like(ce, float("nan")))
            ctx.save_for_backward(logits_tm1, a_arg, lse, target)
        ctx.mark_non_differentiable(target)
        return ce, target

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_ce, _grad_target):
        logits_tm1, a_arg, lse, target = ctx.saved_tensors
        B, A, M = logits_tm1.shape
        if logits_tm1.is_cuda:
            from stoix_amd.ops import ext

            dlogits = torch.empty_like(logits_tm1)
            ext(required=True).c51_loss_bwd(
                grad_ce.float(), logits_tm1, a_arg, lse, target, dlogits
            )
        else:
            rows = torch.arange(B)
            a_ok = (a_arg >= 0) & (a_arg < A)
            a_c = a_arg.clamp(0, A - 1)
            logits_a = logits_tm1.to(target.dtype)[rows, a_c]
            d_a = grad_ce.to(target.dtype).unsqueeze(-1) * (
                torch.exp(logits_a - lse.unsqueeze(-1)) * target.sum(-1, keepdim=True) - target
            )
            dlogits = torch.zeros(B, A, M, dtype=target.dtype)
            dlogits[rows, a_c] = torch.where(a_ok.unsqueeze(-1), d_a, torch.zeros_like(d_a))
            dlogits = dlogits.to(logits_tm1.dtype)
        return dlogits, None, None, None, None, None, None, None


def _c51_ce_composition(
    q_logits_tm1, q_atoms_tm1, a_tm1, r_t, d_t, q_logits_t, q_atoms_t, q_t_selector
) -> Tuple[Tensor, Tensor]:
    """Per-row (ce, target) from the torch ops the categorical losses below
    are made of; autograd differentiates the log-softmax."""
    B = r_t.shape[0]
    if q_atoms_t.dim() == 1:
        q_atoms_t = q_atoms_t.unsqueeze(0).expand(B, -1)
    if q_atoms_tm1.dim() == 1:
        q_atoms_tm1 = q_atoms_tm1.unsqueeze(0).expand(B, -1)
    target_z = r_t.unsqueeze(-1) + d_t.unsqueeze(-1) * q_atoms_t
    probs_t = F.softmax(q_logits_t, dim=-1)
    logits_a = q_logits_tm1
    if q_logits_tm1.dim() == 3:
        if q_t_selector is None:
            best_a = torch.zeros(B, dtype=torch.long, device=probs_t.device)
        else:
            best_a = q_t_selector.argmax(dim=-1)
        if a_tm1 is None:
            a_tm1 = torch.zeros(B, dtype=torch.long, device=probs_t.device)
        probs_t = probs_t.gather(
            1, best_a.view(-1, 1, 1).expand(-1, 1, probs_t.shape[-1])
        ).squeeze(1)
        logits_a = q_logits_tm1.gather(
            1, a_tm1.long().view(-1, 1, 1).expand(-1, 1, q_logits_tm1.shape[-1])
        ).squeeze(1)
    target = categorical_l2_project(target_z, probs_t, q_atoms_tm1[0]).detach()
    return -(target * F.log_softmax(logits_a, dim=-1)).sum(-1), target


def c51_td_cross_entropy(
    q_logits_tm1: Tensor,
    q_atoms_tm1: Tensor,
    a_tm1: Optional[Tensor],
    r_t: Tensor,
    d_t: Tensor,
    q_logits_t: Tensor,
    q_atoms_t: Tensor,
    q_t_selector: Optional[Tensor] = None,
    return_target: bool = False,
):
    """Per-row C51 categorical TD cross-entropy ``ce [B]`` (with
    ``return_target=True``: ``(ce, target [B, M])``).

    Logits are [B, A, atoms] with ``a_tm1 [B]`` and ``q_t_selector [B, A]``
    (double-Q: the selector's argmax picks the target action), or [B, atoms]
    with both None (the categorical_td_learning case, handled as A = 1).
    On the GPU, fp32/bf16 logits with one shared support per side run in the
    two c51.hip kernels: the projection is summed in a fixed order, so ce,
    the target and the gradient are the same on every run. Anything else,
    or STOIX_FUSED_C51=0, runs the torch composition.
    """
    fused = _c51_fused_inputs(
        q_logits_tm1, q_atoms_tm1, a_tm1, q_logits_t, q_atoms_t, q_t_selector
    )
    if fused is not None:
        lt1, z_tm1, lt, z_t = fused
        ce, target = _C51Loss.apply(lt1, z_tm1, a_tm1, r_t, d_t, lt, z_t, q_t_selector)
    else:
        ce, target = _c51_ce_composition(
            q_logits_tm1, q_atoms_tm1, a_tm1, r_t, d_t, q_logits_t, q_atoms_t, q_t_selector
        )
    return (ce, target) if return_target else ce


def _c51_fused_inputs(q_logits_tm1, q_atoms_tm1, a_tm1, q_logits_t, q_atoms_t, q_t_selector):
    """(logits_tm1 [B, A, M], atoms_tm1 [M], logits_t [B, A, N], atoms_t [N])
    as _C51Loss takes them, or None when the inputs go to the torch
    composition instead: knob off, per-row supports, shapes that do not fit,
    or on the GPU a dtype or size outside the kernels' range."""
    if not c51_fused_enabled():
        return None
    lt1, lt = q_logits_tm1, q_logits_t
    if lt1.dim() == 2 and lt.dim() == 2 and a_tm1 is None and q_t_selector is None:
        lt1, lt = lt1.unsqueeze(1), lt.unsqueeze(1)
    z_tm1, z_t = _single_support(q_atoms_tm1), _single_support(q_atoms_t)
    if z_tm1 is None or z_t is None or lt1.dim() != 3 or lt.dim() != 3:
        return None
    A = lt1.shape[1]
    if (
        lt1.shape[:2] != lt.shape[:2]
        or z_tm1.shape[0] != lt1.shape[2]
        or z_t.shape[0] != lt.shape[2]
        or (a_tm1 is None and A != 1)
        or (q_t_selector is None and A != 1)
        or (q_t_selector is not None and q_t_selector.shape != lt1.shape[:2])
    ):
        return None
    if lt1.is_cuda and not _c51_kernel_eligible(lt1, lt):
        return None
    return lt1, z_tm1, lt, z_t


def _c51_route_to_kernel(logits_tm1, atoms_tm1, a_tm1, logits_t, atoms_t, selector) -> bool:
    """Whether a categorical loss below hands its inputs to the HIP kernels."""
    return logits_tm1.is_cuda and (
        _c51_fused_inputs(logits_tm1, atoms_tm1, a_tm1, logits_t, atoms_t, selector)
        is not None
    )


def categorical_double_q_learning(
    q_logits_tm1: Tensor,
    q_atoms_tm1: Tensor,
    a_tm1: Tensor,
    r_t: Tensor,
    d_t: Tensor,
    q_logits_t: Tensor,
    q_atoms_t: Tensor,
    q_t_selector: Tensor,
) -> Tensor:
    """C51 distributional double-Q loss (reference loss.py:81-103).

    Shift/scale target atoms by r + d*z, Cramer-project onto the fixed
    support, cross-entropy against the chosen action's logits.

    Shapes: q_logits [B, A, N], q_atoms [B, N] (or [N]), a/r/d [B],
    q_t_selector [B, A] mean values for argmax.

    On the GPU, eligible inputs run in the fused c51.hip kernels
    (c51_td_cross_entropy).
    """
    if _c51_route_to_kernel(
        q_logits_tm1, q_atoms_tm1, a_tm1, q_logits_t, q_atoms_t, q_t_selector
    ):
        return c51_td_cross_entropy(
            q_logits_tm1, q_atoms_tm1, a_tm1, r_t, d_t, q_logits_t, q_atoms_t, q_t_selector
        ).mean()
    if q_atoms_t.dim() == 1:
        q_atoms_t = q_atoms_t.unsqueeze(0).expand(r_t.shape[0], -1)
    if q_atoms_tm1.dim() == 1:
        q_atoms_tm1 = q_atoms_tm1.unsqueeze(0).expand(r_t.shape[0], -1)
    target_z = r_t.unsqueeze(-1) + d_t.unsqueeze(-1) * q_atoms_t
    best_a = q_t_selector.argmax(dim=-1)
    probs_t = F.softmax(q_logits_t, dim=-1)
    p_best = probs_t.gather(1, best_a.view(-1, 1, 1).expand(-1, 1, probs_t.shape[-1])).squeeze(1)
    target = categorical_l2_project(target_z, p_best, q_atoms_tm1[0]).detach()
    logits_a = q_logits_tm1.gather(
        1, a_tm1.long().view(-1, 1, 1).expand(-1, 1, q_logits_tm1.shape[-1])
    ).squeeze(1)
    return -(target * F.log_softmax(logits_a, dim=-1)).sum(-1).mean()


def categorical_td_learning(
    v_logits_tm1: Tensor,
    v_atoms_tm1: Tensor,
    r_t: Tensor,
    d_t: Tensor,
    v_logits_t: Tensor,
    v_atoms_t: Tensor,
) -> Tensor:
    """Distributional TD for categorical V/Q distributions
    (reference loss.py:166-187; D4PG critic).

    On the GPU, eligible inputs run in the fused c51.hip kernels
    (c51_td_cross_entropy with A = 1)."""
    if _c51_route_to_kernel(v_logits_tm1, v_atoms_tm1, None, v_logits_t, v_atoms_t, None):
        return c51_td_cross_entropy(
            v_logits_tm1, v_atoms_tm1, None, r_t, d_t, v_logits_t, v_atoms_t
        ).mean()
    if v_atoms_t.dim() == 1:
        v_atoms_t = v_atoms_t.unsqueeze(0).expand(r_t.shape[0], -1)
    if v_atoms_tm1.dim() == 1:
        v_atoms_tm1 = v_atoms_tm1.unsqueeze(0).expand(r_t.shape[0], -1)
    target_z = r_t.unsqueeze(-1) + d_t.unsqueeze(-1) * v_atoms_t
    probs_t = F.softmax(v_logits_t, dim=-1)
    target = categorical_l2_project(target_z, probs_t, v_atoms_tm1[0]).detach()
    return -(target * F.log_softmax(v_logits_tm1, dim=-1)).sum(-1).mean()


def munchausen_q_learning(
    q_tm1: Tensor,
    a_tm1: Tensor,
    r_t: Tensor,
    d_t: Tensor,
    q_t: Tensor,
    q_target_tm1: Tensor,
    entropy_temperature: float,
    munchausen_coefficient: float,
    clip_value_min: float,
    huber_loss_parameter: float = 0.0,
) -> Tensor:
    """Munchausen DQN loss (Vieillard et al. 2020; reference loss.py:190-223).

    bonus = alpha * clip(tau * log_pi_target(a_tm1), min, 0)
    soft_target = sum_a pi_t(a) * (q_t(a) - tau * log pi_t(a))
    target = r + bonus + d * soft_target.
    """
    tau = entropy_temperature
    logits_target_tm1 = q_target_tm1 / tau
    log_pi_tm1 = F.log_softmax(logits_target_tm1, dim=-1)
    bonus = munchausen_coefficient * torch.clamp(
        tau * log_pi_tm1.gather(-1, a_tm1.long().unsqueeze(-1)).squeeze(-1),
        min=clip_value_min,
        max=0.0,
    )
    log_pi_t = F.log_softmax(q_t / tau, dim=-1)
    pi_t = log_pi_t.exp()
    soft_v = (pi_t * (q_t - tau * log_pi_t)).sum(-1)
    target = (r_t + bonus + d_t * soft_v).detach()
    q_a = q_tm1.gather(-1, a_tm1.long().unsqueeze(-1)).squeeze(-1)
    return _huber(target - q_a, huber_loss_parameter).mean()


def quantile_regression_loss(
    dist_src: Tensor,
    tau_src: Tensor,
    dist_target: Tensor,
    huber_param: float = 1.0,
) -> Tensor:
    """Quantile-regression (pinball) loss (reference loss.py:226-265).

    dist_src [B, N] quantile estimates with thresholds tau_src [N] (or [B, N]);
    dist_target [B, M] target samples.
    """
    if tau_src.dim() == 1:
        tau_src = tau_src.unsqueeze(0).expand(dist_src.shape[0], -1)
    # pairwise TD errors: target_j - src_i -> [B, N, M]
    delta = dist_target.detach().unsqueeze(1) - dist_src.unsqueeze(2)
    weight = (tau_src.unsqueeze(2) - (delta < 0).to(delta.dtype)).abs()
    if huber_param > 0:
        loss = _huber(delta, huber_param) / huber_param
    else:
        loss = delta.abs()
    return (weight * loss).mean(dim=2).sum(dim=1).mean()


def quantile_q_learning(
    dist_q_tm1: Tensor,
    tau_q_tm1: Tensor,
    a_tm1: Tensor,
    r_t: Tensor,
    d_t: Tensor,
    dist_q_t_selector: Tensor,
    dist_q_t: Tensor,
    huber_param: float = 1.0,
) -> Tensor:
    """QR-DQN loss (reference loss.py:268-314).

    dist_q [B, N, A]; selector distribution picks argmax over mean-quantile
    values; target dist = r + d * dist_q_t[:, :, a*].
    """
    q_a = dist_q_tm1.gather(
        2, a_tm1.long().view(-1, 1, 1).expand(-1, dist_q_tm1.shape[1], 1)
    ).squeeze(-1)
    best_a = dist_q_t_selector.mean(dim=1).argmax(dim=-1)
    target_dist = dist_q_t.gather(
        2, best_a.view(-1, 1, 1).expand(-1, dist_q_t.shape[1], 1)
    ).squeeze(-1)
    target = (r_t.unsqueeze(-1) + d_t.unsqueeze(-1) * target_dist).detach()
    return quantile_regression_loss(q_a, tau_q_tm1, target, huber_param)
