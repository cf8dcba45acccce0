"""CPU: the SAC loss functions of ops/losses.py are the expressions ff_sac.py
used to hold inline, bit for bit and with either STOIX_FUSED_SAC setting, and
AffineTanhTransformedDistribution.sample_and_log_prob is unchanged there."""
import math

import pytest
import torch
import torch.nn.functional as F


@pytest.mark.parametrize("knob", ["0", "1"])
@pytest.mark.parametrize("Q,B", [(1, 1), (2, 37)])
def test_sac_losses_equal_the_former_inline_expressions(monkeypatch, knob, Q, B):
    from stoix_amd.ops.losses import sac_actor_alpha_losses, sac_critic_loss

    monkeypatch.setenv("STOIX_FUSED_SAC", knob)
    g = torch.Generator().manual_seed(3)
    q_pred, q_next, q_new = (torch.randn(Q, B, generator=g) for _ in range(3))
    logp_next, logp_new, reward = (torch.randn(B, generator=g) * 5 for _ in range(3))
    discount = (torch.rand(B, generator=g) > 0.2).float()
    gamma, target_entropy = 0.99, -3.0

    def grads(fn):
        la = torch.tensor(-0.7, requires_grad=True)
        leaves = [la] + [t.clone().requires_grad_(True) for t in (q_pred, q_new, logp_new)]
        outs = fn(*leaves)
        (outs[0] + outs[2] + outs[3]).backward()
        return [o.detach() for o in outs] + [t.grad for t in leaves]

    def inline(la, qp, qn, lpn):  # ff_sac.py before the functions existed
        alpha = la.exp().detach()
        with torch.no_grad():
            target = reward + gamma * discount * (q_next.min(dim=0).values - alpha * logp_next)
        q_loss = 0.5 * ((qp - target.unsqueeze(0)) ** 2).mean()
        actor_loss = (alpha * lpn - qn.min(dim=0).values).mean()
        alpha_loss = -(la * (lpn + target_entropy).detach()).mean()
        return q_loss, target, actor_loss, alpha_loss, -lpn.mean().detach()

    def functions(la, qp, qn, lpn):
        q_loss, target = sac_critic_loss(qp, q_next, logp_next, reward, discount, la, gamma)
        return (q_loss, target, *sac_actor_alpha_losses(qn, lpn, la, target_entropy))

    for got, want in zip(grads(functions), grads(inline)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("knob", ["0", "1"])
def test_sample_and_log_prob_on_the_cpu_is_unchanged(monkeypatch, knob):
    from stoix_amd.networks.distributions import AffineTanhTransformedDistribution

    monkeypatch.setenv("STOIX_FUSED_SAC", knob)
    loc = torch.linspace(-3, 3, 15).reshape(5, 3).requires_grad_(True)
    scale = torch.linspace(0.05, 1.5, 15).reshape(5, 3)
    d = AffineTanhTransformedDistribution(loc, scale, -0.4, 2.0)
    a, lp = d.sample_and_log_prob(torch.Generator().manual_seed(11))
    sa, sh = (2.0 - -0.4) / 2.0, (2.0 + -0.4) / 2.0
    u = loc + scale * torch.randn(loc.shape, generator=torch.Generator().manual_seed(11))
    log_det = 2.0 * (math.log(2.0) - u - F.softplus(-2.0 * u)) + math.log(sa)
    base = -((u - loc) ** 2) / (2 * scale**2) - scale.log() - 0.5 * math.log(2 * math.pi)
    assert torch.equal(a, torch.tanh(u) * sa + sh)
    assert torch.equal(lp, (base - log_det).sum(-1))
    assert lp.grad_fn is not None and type(lp.grad_fn).__name__ == "SumBackward1"
