"""GPU tests of the fused Gaussian actor (ops/csrc/actor_mlp.hip) against plain
fp64 torch on the CPU.

Kernel bounds are the per-element rule of tests/test_qens_gpu.py, applied layer
by layer on the layer's own input as the kernel stored it (so a ReLU kink of an
earlier layer cannot enter): for a sum of L fp32 products
``|got - ref64| <= (L + c) * 2^-24 * sum |terms|``. Forward: c = 3 (bias add);
SiLU outputs ``1.1 * bound_Z + 2^-21 |H|``. ``scale`` and ``dspre`` are a few
roundings and one exp / log1p of the stored ``spre``: ``2^-21 |ref|``.
Backward: c = 16 for the act' factor, times 1.1 = sup |silu'| for SiLU; ReLU
takes its mask from the stored H, as the kernel does. The module test uses the
rule of tests/test_sac_fused_gpu.py:
``max|fused - fp64| <= 2 max|fp32 chain - fp64| + 1 fp32 ulp``.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

U = 2.0**-24
ACTS = {"silu": 1, "relu": 2}
MIN_SCALE = 1e-3

# (S, K0, widths, A, act)
CASES = [
    (1, 5, [16], 1, "relu"),
    (17, 27, [48, 16], 17, "silu"),
    (130, 40, [256, 256], 64, "relu"),
    (130, 27, [32, 64, 16, 48], 17, "silu"),
    (17, 5, [256, 256], 1, "silu"),
    (130, 40, [48, 16], 64, "silu"),
    (1, 27, [32, 64, 16, 48], 64, "relu"),
    (17, 40, [16], 17, "relu"),
    (130, 5, [48, 16], 1, "relu"),
    (130, 300, [256, 256], 17, "silu"),  # a second chunk of the staged input
]


def _ext():
    from stoix_amd import ops

    return ops.ext(required=True)


def _check(name, got, ref, bound):
    err = (got.detach().cpu().double() - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item() if (bound > 0).any() else 0.0
    print(f"{name}: max err {err.max().item():.3e}, worst err/bound {worst:.3f}")
    assert got.shape == ref.shape and (err <= bound).all(), name


def _act64(z, act):
    return torch.relu(z) if act == "relu" else z * torch.sigmoid(z)


def _act_grad64(aux, act):
    """act' from the stored H (ReLU) or Z (SiLU), and the factor of the bound."""
    if act == "relu":
        return (aux > 0).double(), (aux > 0).double()
    s = torch.sigmoid(aux)
    return s * (1 + aux * (1 - s)), torch.full_like(aux, 1.1)


@requires_gpu
@pytest.mark.parametrize("S,K0,widths,A,act", CASES)
def test_kernels_match_fp64_layer_by_layer(S, K0, widths, A, act):
    ext = _ext()
    g = torch.Generator().manual_seed(S + 7 * K0 + 31 * A + len(widths))
    r = lambda *s: torch.randn(*s, generator=g)
    dims = [K0, *widths]
    Ws = [r(n, k) / k**0.5 for k, n in zip(dims, dims[1:])]
    bs = [0.1 * r(n) for n in widths]
    Wl, Wsc = r(A, dims[-1]) / dims[-1] ** 0.5, r(A, dims[-1]) / dims[-1] ** 0.5
    bl, bsc = 0.1 * r(A), 0.1 * r(A)
    if A > 1:
        bsc[::3] += 25.0  # spre above softplus' threshold of 20 on these columns
    X, dloc, dscale = r(S, K0), r(S, A), r(S, A)
    dev = lambda ts: [t.cuda() for t in ts]
    new = lambda *s: torch.full(s, float("nan"), device="cuda")
    net = (dev(Ws), dev(bs), Wl.cuda(), bl.cuda(), Wsc.cuda(), bsc.cuda())

    loc, scale, spre = new(S, A), new(S, A), new(S, A)
    Hs = [new(S, n) for n in widths]
    Zs = [new(S, n) for n in widths] if act == "silu" else []
    assert ext.actor_mlp_fwd(X.cuda(), *net, MIN_SCALE, ACTS[act], loc, scale, spre, Hs, Zs)
    h = X.double()
    for l, (W, b) in enumerate(zip(Ws, bs)):
        z64 = h @ W.double().T + b.double()
        bz = (dims[l] + 3) * U * (h.abs() @ W.double().abs().T + b.double().abs())
        if act == "silu":
            _check(f"Z{l}", Zs[l], z64, bz)
            _check(f"H{l}", Hs[l], _act64(z64, act), 1.1 * bz + 2.0**-21 * _act64(z64, act).abs())
        else:
            _check(f"H{l}", Hs[l], _act64(z64, act), bz)
        h = Hs[l].cpu().double()
    for name, got, W, b in (("loc", loc, Wl, bl), ("spre", spre, Wsc, bsc)):
        _check(name, got, h @ W.double().T + b.double(),
               (dims[-1] + 3) * U * (h.abs() @ W.double().abs().T + b.double().abs()))
    sp = spre.cpu().double()
    assert A == 1 or ((sp > 20).any() and (sp < 20).any())
    scale64 = torch.where(sp > 20, sp, F.softplus(sp)) + MIN_SCALE
    _check("scale", scale, scale64, 2.0**-21 * scale64)

    # without a backward to follow: the same loc and scale, nothing else stored
    loc2, scale2 = new(S, A), new(S, A)
    assert ext.actor_mlp_fwd(X.cuda(), *net, MIN_SCALE, ACTS[act], loc2, scale2, torch.empty(0, device="cuda"), [], [])
    assert torch.equal(loc2, loc) and torch.equal(scale2, scale)

    dZs, dZh = [new(S, n) for n in widths], new(2, S, A)
    aux = Zs if act == "silu" else Hs
    assert ext.actor_mlp_dgrad(dloc.cuda(), dscale.cuda(), spre, K0, *net, ACTS[act], aux, dZs, dZh)
    assert torch.equal(dZh[0].cpu(), dloc)
    dspre64 = dscale.double() * torch.where(sp > 20, torch.ones_like(sp), torch.sigmoid(sp))
    _check("dspre", dZh[1], dspre64, 2.0**-21 * dspre64.abs())
    dz = torch.cat([dZh[0], dZh[1]], -1).cpu().double()  # [S, 2A], as the kernel stored it
    W = torch.cat([Wl, Wsc], 0).double()
    for l in range(len(widths) - 1, -1, -1):
        grad, factor = _act_grad64(aux[l].cpu().double(), act)
        _check(f"dZ{l}", dZs[l], (dz @ W) * grad, (W.shape[0] + 16) * U * (dz.abs() @ W.abs()) * factor)
        dz, W = dZs[l].cpu().double(), Ws[l].double()


# ------------------------------------------------------------ module level

OBS, ACT_DIM, S_MOD = 27, 5, 130
# ReLU: a seed at which the fp64 reference on the CPU has no hidden
# pre-activation within 1e-4 of the kink (the nearest is 5.4e-4 away)
MODULE_SEED = {"relu": 25, "silu": 0}


def _actor(act, widths=(48, 32), layer_norm=False):
    from stoix_amd.networks.base import FeedForwardActor
    from stoix_amd.networks.heads import NormalAffineTanhDistributionHead
    from stoix_amd.networks.torso import MLPTorso

    torch.manual_seed(MODULE_SEED[act])
    torso = MLPTorso(OBS, list(widths), activation=act, use_layer_norm=layer_norm)
    actor = FeedForwardActor(torso, NormalAffineTanhDistributionHead(torso.output_dim, ACT_DIM, -1.0, 1.0))
    for p in actor.parameters():
        if p.dim() == 1:
            nn.init.normal_(p, std=0.1)
    return actor, torch.randn(S_MOD, OBS), torch.randn(S_MOD, ACT_DIM), torch.randn(S_MOD, ACT_DIM)


def _outputs_and_grads(actor, obs, w1, w2):
    dist = actor(obs)
    loc, scale = dist.base.loc, dist.base.scale
    grads = torch.autograd.grad((loc * w1 + scale * w2).sum(), list(actor.parameters()))
    return [loc.detach(), scale.detach(), *grads]


@requires_gpu
@pytest.mark.parametrize("act", ["relu", "silu"])
def test_module_matches_fp64_autograd_and_captures(act, monkeypatch):
    from stoix_amd.ops.actor_mlp import actor_route_to_kernel

    monkeypatch.setenv("STOIX_FUSED_ACTOR", "1")
    actor, obs, w1, w2 = _actor(act)
    ref = _outputs_and_grads(copy.deepcopy(actor).double(), obs.double(), w1.double(), w2.double())
    chain = _outputs_and_grads(actor, obs, w1, w2)  # on the CPU: the module chain
    if act == "relu":  # a condition on the reference, not a tolerance
        h = obs.double()
        for mod in copy.deepcopy(actor).double().torso.net:
            if isinstance(mod, nn.Linear):
                assert mod(h).abs().min().item() >= 1e-4, "pre-activation too close to the ReLU kink"
            h = mod(h)

    dev = copy.deepcopy(actor).cuda()
    obs_d, w1_d, w2_d = obs.cuda(), w1.cuda(), w2.cuda()
    assert actor_route_to_kernel(dev, obs_d)
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _outputs_and_grads(dev, obs_d, w1_d, w2_d)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    names = ["loc", "scale", *(n for n, _ in actor.named_parameters())]
    for name, k, r, c in zip(names, got, ref, chain):
        err, err_chain = (k.cpu().double() - r).abs().max().item(), (c.double() - r).abs().max().item()
        ulp = float(np.spacing(np.float32(r.abs().max().item())))
        print(f"{act} {name}: fused {err:.3e} chain {err_chain:.3e} ratio {err / max(err_chain, 1e-300):.3f}")
        assert k.shape == r.shape and err <= 2 * err_chain + ulp, name

    # captured once, replayed twice: the eager result's bits both times
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _outputs_and_grads(dev, obs_d, w1_d, w2_d)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _outputs_and_grads(dev, obs_d, w1_d, w2_d)
    for _ in range(2):
        for t in out:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, got))


@requires_gpu
@pytest.mark.parametrize("case", ["layer_norm", "width 72", "width 272", "obs grad", "autocast", "knob off"])
def test_ineligible_cases_keep_the_module_chain_bit_for_bit(case, monkeypatch):
    from stoix_amd.ops.actor_mlp import actor_route_to_kernel

    monkeypatch.setenv("STOIX_FUSED_ACTOR", "0" if case == "knob off" else "1")
    widths = {"width 72": (72, 32), "width 272": (272, 32)}.get(case, (48, 32))
    actor, obs, _, _ = _actor("silu", widths, layer_norm=case == "layer_norm")
    actor, obs = actor.cuda(), obs.cuda().requires_grad_(case == "obs grad")
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=case == "autocast"):
        assert not actor_route_to_kernel(actor, obs)
        dist, want = actor(obs), actor.action_head(actor.torso(obs))
    assert torch.equal(dist.base.loc, want.base.loc) and torch.equal(dist.base.scale, want.base.scale)


@requires_gpu
def test_sac_update_step_runs_on_the_fused_actor(monkeypatch):
    from stoix_amd import envs as environments
    from stoix_amd.config import compose
    from stoix_amd.ops.actor_mlp import actor_route_to_kernel
    from stoix_amd.systems.sac.ff_sac import SACLearner
    from stoix_amd.utils.total_timestep_checker import check_total_timesteps

    monkeypatch.setenv("STOIX_FUSED_ACTOR", "1")
    cfg = compose(
        "default/anakin/default_ff_sac.yaml",
        ["env=brax/humanoid", "arch.total_num_envs=64", "arch.total_timesteps=null",
         "arch.num_updates=2", "arch.num_evaluation=1", "system.rollout_length=2",
         "system.batch_size=64", "system.buffer_size=2048", "system.warmup_steps=16",
         "system.epochs=1", "logger.loggers=[]", "logger.checkpointing.save_model=false"],
    )
    cfg.arch.n_devices = 1
    check_total_timesteps(cfg)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    learner = SACLearner(cfg, environments.make_single(cfg, 64, dev, seed=0), dev)
    obs_dim = learner.actor.torso.net[0].in_features
    assert actor_route_to_kernel(learner.actor, torch.zeros(64, obs_dim, device=dev))
    before = [p.detach().clone() for p in learner.actor.parameters()]
    learner.update_step()
    torch.cuda.synchronize()
    for group in ("actor", "q_online", "q_target"):
        assert all(torch.isfinite(p).all() for p in getattr(learner, group).parameters()), group
    assert all(not torch.equal(p, b) for p, b in zip(learner.actor.parameters(), before))
