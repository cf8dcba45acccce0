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
these references (tests/test_losses.py). On the GPU the distributional
losses run in HIP: the categorical ones in c51.hip, the quantile ones in
qr.hip (quantile_q_learning_rows is the per-row entry point).
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


# -------------------------------------------------- fused QR loss (qr.hip)

_QR_MAX_QUANTILES = 1024
_QR_MAX_ACTIONS = 64


def qr_fused_enabled() -> bool:
    """STOIX_FUSED_QR=0 forces the torch composition (A/B timing)."""
    return os.environ.get("STOIX_FUSED_QR", "1") != "0"


def _qr_route_to_kernel(src, tau, tgt, sel=None, rows=()) -> bool:
    """Whether a quantile loss below hands its inputs to the HIP kernels:
    knob on, [B, quantiles, A] fp32/bf16 GPU tensors within the kernels' size
    limits, tau [N] or [B, N] that needs no gradient, per-row vectors [B]."""
    if not qr_fused_enabled() or not isinstance(src, Tensor) or src.dim() != 3:
        return False
    B, N, A = src.shape
    for t in (src, tgt) if sel is None else (src, tgt, sel):
        if not t.is_cuda or t.dtype not in (torch.float32, torch.bfloat16):
            return False
        if t.dim() != 3 or t.shape[0] != B or t.shape[2] != A:
            return False
        if not 1 <= t.shape[1] <= _QR_MAX_QUANTILES:
            return False
    if B < 1 or not 1 <= A <= _QR_MAX_ACTIONS:
        return False
    if not tau.is_cuda or not tau.is_floating_point() or tau.shape not in ((N,), (B, N)):
        return False
    if tau.requires_grad and torch.is_grad_enabled():
        return False
    return all(isinstance(v, Tensor) and v.is_cuda and v.shape == (B,) for v in rows)


class _QRLoss(torch.autograd.Function):
    """Per-row quantile-regression loss with its closed-form gradient to the
    source quantiles, GPU only: forward is qr_loss_fwd (which also leaves
    d loss / d th in ``gth [B, N]``), backward is qr_loss_bwd. Nothing flows
    to tau, the target samples, the selector, r or d.

    ``src [B, N, A]``, ``tgt [B, M, A]``, ``sel [B, Ns, A]`` or None (A = 1),
    ``a`` int [B] or None (A = 1), ``r``/``d`` [B] or both None (targets taken
    as they are)."""

    @staticmethod
    def forward(ctx, src, tau, a, r, d, sel, tgt, huber_param):
        from stoix_amd.ops import ext

        B, N, A = src.shape
        src = src.contiguous()
        dev = src.device
        empty = torch.empty(0, dtype=torch.float32, device=dev)
        tau = tau.float()
        if N > 1 and tau.stride(-1) != 1:
            tau = tau.contiguous()
        a_arg = torch.empty(0, dtype=torch.long, device=dev) if a is None else a.long()
        loss = torch.empty(B, dtype=torch.float32, device=dev)
        gth = torch.empty(B, N, dtype=torch.float32, device=dev)
        ext(required=True).qr_loss_fwd(
            src,
            tau,  # [N], or [B, N] read through its row stride
            a_arg,  # per-row vectors may be strided views
            empty if r is None else r.float(),
            empty if d is None else d.float(),
            empty if sel is None else sel.contiguous(),
            tgt.contiguous(),
            loss,
            gth,
            float(huber_param),
        )
        ctx.save_for_backward(gth, a_arg)
        ctx.src_meta = (src.shape, src.dtype)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        from stoix_amd.ops import ext

        gth, a_arg = ctx.saved_tensors
        shape, dtype = ctx.src_meta
        dsrc = torch.empty(shape, dtype=dtype, device=gth.device)
        ext(required=True).qr_loss_bwd(grad_loss.float(), gth, a_arg, dsrc)
        return dsrc, None, None, None, None, None, None, None


def _qr_rows_composition(dist_src, tau_src, dist_target, huber_param) -> Tensor:
    """Per-row loss [B] from the torch ops quantile_regression_loss is made
    of (its lines without the final mean)."""
    if tau_src.dim() == 1:
        tau_src = tau_src.unsqueeze(0).expand(dist_src.shape[0], -1)
    delta = dist_target.detach().unsqueeze(1) - dist_src.unsqueeze(2)
    weight = (tau_src.unsqueeze(2) - (delta < 0).to(delta.dtype)).abs()
    if huber_param > 0:
        loss = _huber(delta, huber_param) / huber_param
    else:
        loss = delta.abs()
    return (weight * loss).mean(dim=2).sum(dim=1)


def quantile_q_learning_rows(
    dist_q_tm1: Tensor,
    tau_q_tm1: Tensor,
    a_tm1: Tensor,
    r_t: Tensor,
    d_t: Tensor,
    dist_q_t_selector: Tensor,
    dist_q_t: Tensor,
    huber_param: float = 1.0,
) -> Tensor:
    """Per-row QR-DQN loss ``[B]``; ``quantile_q_learning`` is its mean. For
    callers that weight the rows (importance weights, priorities).

    dist_q [B, quantiles, A], tau [N] or [B, N], a/r/d [B]. On the GPU,
    fp32/bf16 inputs with at most 1024 quantiles and 64 actions run in the
    two qr.hip kernels (fp32 rows; the gradient in dist_q_tm1's dtype, summed
    in a fixed order, so the same bits on every run). Anything else, or
    STOIX_FUSED_QR=0, runs the torch composition.
    """
    if _qr_route_to_kernel(
        dist_q_tm1, tau_q_tm1, dist_q_t, dist_q_t_selector, (a_tm1, r_t, d_t)
    ):
        return _QRLoss.apply(
            dist_q_tm1, tau_q_tm1, a_tm1, r_t, d_t, dist_q_t_selector, dist_q_t, huber_param
        )
    q_a = dist_q_tm1.gather(
        2, a_tm1.long().view(-1, 1, 1).expand(-1, dist_q_tm1.shape[1], 1)
    ).squeeze(-1)
    best_a = dist_q_t_selector.mean(dim=1).argmax(dim=-1)
    target_dist = dist_q_t.gather(
        2, best_a.view(-1, 1, 1).expand(-1, dist_q_t.shape[1], 1)
    ).squeeze(-1)
    target = (r_t.unsqueeze(-1) + d_t.unsqueeze(-1) * target_dist).detach()
    return _qr_rows_composition(q_a, tau_q_tm1, target, huber_param)


def quantile_regression_loss(
    dist_src: Tensor,
    tau_src: Tensor,
    dist_target: Tensor,
    huber_param: float = 1.0,
) -> Tensor:
    """Quantile-regression (pinball) loss (reference loss.py:226-265).

    dist_src [B, N] quantile estimates with thresholds tau_src [N] (or [B, N]);
    dist_target [B, M] target samples.

    On the GPU, eligible inputs run in the fused qr.hip kernels (as A = 1,
    see quantile_q_learning_rows).
    """
    if (
        dist_src.dim() == 2
        and dist_target.dim() == 2
        and _qr_route_to_kernel(dist_src.unsqueeze(-1), tau_src, dist_target.unsqueeze(-1))
    ):
        return _QRLoss.apply(
            dist_src.unsqueeze(-1), tau_src, None, None, None, None,
            dist_target.detach().unsqueeze(-1), huber_param,
        ).mean()
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

    On the GPU, eligible inputs run in the fused qr.hip kernels
    (quantile_q_learning_rows).
    """
    if _qr_route_to_kernel(
        dist_q_tm1, tau_q_tm1, dist_q_t, dist_q_t_selector, (a_tm1, r_t, d_t)
    ):
        return _QRLoss.apply(
            dist_q_tm1, tau_q_tm1, a_tm1, r_t, d_t, dist_q_t_selector, dist_q_t, huber_param
        ).mean()
    q_a = dist_q_tm1.gather(
        2, a_tm1.long().view(-1, 1, 1).expand(-1, dist_q_tm1.shape[1], 1)
    ).squeeze(-1)
    best_a = dist_q_t_selector.mean(dim=1).argmax(dim=-1)
    target_dist = dist_q_t.gather(
        2, best_a.view(-1, 1, 1).expand(-1, dist_q_t.shape[1], 1)
    ).squeeze(-1)
    target = (r_t.unsqueeze(-1) + d_t.unsqueeze(-1) * target_dist).detach()
    return quantile_regression_loss(q_a, tau_q_tm1, target, huber_param)


# ----------------------------- fused SAC loss rows (tanh_normal.hip)

_SAC_MAX_CRITICS = 4


def sac_fused_enabled() -> bool:
    """STOIX_FUSED_SAC=0 forces the torch chain on the GPU for the
    tanh-Normal sample and for the two SAC loss functions below (A/B timing)."""
    return os.environ.get("STOIX_FUSED_SAC", "1") != "0"


def _sac_route_to_kernel(q: Tensor, log_alpha: Tensor, rows=(), twin=None) -> bool:
    """Whether a SAC loss below hands its inputs to the HIP kernels: knob on,
    fp32 GPU critic values [Q, B] with 1 <= Q <= 4 (``twin`` of the same
    shape), a one-element fp32 GPU log_alpha and fp32 GPU per-row vectors [B]."""
    if not sac_fused_enabled() or not isinstance(q, Tensor) or q.dim() != 2:
        return False
    Q, B = q.shape
    if not 1 <= Q <= _SAC_MAX_CRITICS or B < 1:
        return False
    for t in (q,) if twin is None else (q, twin):
        if not t.is_cuda or t.dtype != torch.float32 or t.shape != (Q, B):
            return False
    if not (
        isinstance(log_alpha, Tensor)
        and log_alpha.is_cuda
        and log_alpha.dtype == torch.float32
        and log_alpha.numel() == 1
    ):
        return False
    return all(
        isinstance(v, Tensor) and v.is_cuda and v.dtype == torch.float32 and v.shape == (B,)
        for v in rows
    )


class _SACCriticRows(torch.autograd.Function):
    """Soft TD target and per-row twin-Q squared error, GPU only
    (sac_critic_rows_kernel); the gradient goes to q_pred alone, through the
    saved ``q_pred - target`` (sac_rows_bwd_kernel)."""

    @staticmethod
    def forward(ctx, q_pred, q_next, logp_next, r_t, d_t, log_alpha, gamma):
        from stoix_amd.ops import ext

        Q, B = q_pred.shape
        dev = q_pred.device
        target = torch.empty(B, dtype=torch.float32, device=dev)
        rows = torch.empty(B, dtype=torch.float32, device=dev)
        dq = torch.empty(Q, B, dtype=torch.float32, device=dev)
        ext(required=True).sac_critic_rows(
            q_pred.contiguous(), q_next.contiguous(), logp_next, r_t, d_t,  # rows may be strided
            log_alpha.detach(), float(gamma), target, rows, dq,
        )
        ctx.save_for_backward(dq)
        ctx.mark_non_differentiable(target)
        return rows, target

    @staticmethod
    @once_differentiable
    def backward(ctx, g_rows, _g_target):
        from stoix_amd.ops import ext

        (dq,) = ctx.saved_tensors
        dq_pred = torch.empty_like(dq)
        ext(required=True).sac_critic_rows_bwd(g_rows, dq, dq_pred)
        return dq_pred, None, None, None, None, None, None


class _SACActorRows(torch.autograd.Function):
    """Per-row actor term, temperature dual term and entropy, GPU only
    (sac_actor_rows_kernel). Gradients: the arg-min critic of q_new and
    logp_new from the actor term (alpha a constant), log_alpha from the dual
    (logp_new a constant), all from sac_rows_bwd_kernel."""

    @staticmethod
    def forward(ctx, q_new, logp_new, log_alpha, target_entropy):
        from stoix_amd.ops import ext

        Q, B = q_new.shape
        dev = q_new.device
        actor_rows, alpha_rows, entropy_rows = (
            torch.empty(B, dtype=torch.float32, device=dev) for _ in range(3)
        )
        argmin = torch.empty(B, dtype=torch.int32, device=dev)
        ext(required=True).sac_actor_rows(
            q_new.contiguous(), logp_new, log_alpha, float(target_entropy),
            actor_rows, alpha_rows, argmin, entropy_rows,
        )
        ctx.save_for_backward(argmin, logp_new, log_alpha)
        ctx.target_entropy = float(target_entropy)
        ctx.Q = Q
        ctx.mark_non_differentiable(entropy_rows)
        return actor_rows, alpha_rows, entropy_rows

    @staticmethod
    @once_differentiable
    def backward(ctx, g_actor, g_alpha, _g_entropy):
        from stoix_amd.ops import ext

        argmin, logp_new, log_alpha = ctx.saved_tensors
        B = logp_new.shape[0]
        dev = logp_new.device
        dq_new = torch.empty(ctx.Q, B, dtype=torch.float32, device=dev)
        dlogp_new = torch.empty(B, dtype=torch.float32, device=dev)
        dla_rows = torch.empty(B, dtype=torch.float32, device=dev)
        ext(required=True).sac_actor_rows_bwd(
            g_actor, g_alpha, argmin, logp_new, log_alpha, ctx.target_entropy,
            dq_new, dlogp_new, dla_rows,
        )
        dla = dla_rows.sum().reshape(log_alpha.shape) if ctx.needs_input_grad[2] else None
        return dq_new, dlogp_new, dla, None


def sac_critic_loss(
    q_pred: Tensor,
    q_next: Tensor,
    logp_next: Tensor,
    r_t: Tensor,
    d_t: Tensor,
    log_alpha: Tensor,
    gamma: float,
) -> Tuple[Tensor, Tensor]:
    """SAC critic loss and its soft TD target (Haarnoja et al. 2018).

    ``q_pred`` / ``q_next`` [Q, B] (online critics at the stored action,
    target critics at a fresh next action), ``logp_next`` / ``r_t`` / ``d_t``
    [B]: ``target = r + gamma * d * (min_q q_next - alpha * logp_next)``, a
    constant; ``loss = 0.5 * mean((q_pred - target)^2)`` over all Q * B.
    Returns ``(loss, target)``.

    On the GPU, fp32 inputs with at most 4 critics run in tanh_normal.hip
    (one kernel forward, one backward, log_alpha read on the device); the CPU,
    anything else, or STOIX_FUSED_SAC=0 runs the torch expressions.
    """
    if _sac_route_to_kernel(q_pred, log_alpha, (logp_next, r_t, d_t), twin=q_next):
        rows, target = _SACCriticRows.apply(
            q_pred, q_next.detach(), logp_next.detach(), r_t, d_t, log_alpha, gamma
        )
        return rows.mean() / q_pred.shape[0], target
    alpha = log_alpha.exp().detach()
    with torch.no_grad():
        target = r_t + gamma * d_t * (q_next.min(dim=0).values - alpha * logp_next)
    return 0.5 * ((q_pred - target.unsqueeze(0)) ** 2).mean(), target


def sac_actor_alpha_losses(
    q_new: Tensor,
    logp_new: Tensor,
    log_alpha: Tensor,
    target_entropy: float,
) -> Tuple[Tensor, Tensor, Tensor]:
    """SAC actor loss ``mean(alpha * logp_new - min_q q_new)`` (alpha a
    constant), temperature dual ``-mean(log_alpha * sg(logp_new + H*))`` and
    the entropy estimate ``-mean(logp_new)`` (detached).

    ``q_new`` [Q, B] are the online critics at the reparameterised action,
    ``logp_new`` [B] its log-probability. Returns
    ``(actor_loss, alpha_loss, entropy)``. Routed as sac_critic_loss.
    """
    if _sac_route_to_kernel(q_new, log_alpha, (logp_new,)):
        actor_rows, alpha_rows, entropy_rows = _SACActorRows.apply(
            q_new, logp_new, log_alpha, target_entropy
        )
        return actor_rows.mean(), alpha_rows.mean(), entropy_rows.mean()
    alpha = log_alpha.exp().detach()
    actor_loss = (alpha * logp_new - q_new.min(dim=0).values).mean()
    alpha_loss = -(log_alpha * (logp_new + target_entropy).detach()).mean()
    return actor_loss, alpha_loss, -logp_new.mean().detach()
