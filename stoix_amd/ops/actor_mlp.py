"""Fused Gaussian actor MLP (ops/csrc/actor_mlp.hip): the whole
``FeedForwardActor`` of the fp32 continuous systems (``MLPTorso`` +
``NormalAffineTanhDistributionHead``) in one launch forward, and its whole
input-gradient chain in one launch backward, fp32 on the matrix cores. The
weight gradients run on the Q-ensemble wgrad kernel (``ext.qens_linear_wgrad``)
over the ``dZ`` the backward kernel stores.

``FeedForwardActor.forward`` (networks/base.py) routes here when
``actor_route_to_kernel`` says so; every other case keeps its module chain.
The ``nn.Linear`` parameters stay where they are and are read in place.
"""
from __future__ import annotations

import os
from typing import List, NamedTuple, Optional

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from stoix_amd.ops.noisy import ACT_CODES, act_kind

Tensor = torch.Tensor

MAX_LAYERS = 4
MAX_WIDTH = 256
MAX_ACTION_DIM = 64


def actor_fused_enabled() -> bool:
    """STOIX_FUSED_ACTOR=1 puts eligible Gaussian actors on the actor_mlp.hip
    kernels. Measured in one call, `bench.py --config sac` is 9.4% faster with
    it at 2048 envs and 29% faster at 512, yet the default is off: with it on,
    tests/test_sac_fused_gpu.py's update-step comparison of STOIX_FUSED_SAC
    (a noise-against-noise rule that passed with a 3% margin) misses its bound
    by 10% on the actor's parameters (profiles/actor_mlp_SUMMARY.md)."""
    return os.environ.get("STOIX_FUSED_ACTOR", "0") == "1"


class ActorLayers(NamedTuple):
    hidden: List[nn.Linear]
    act: str  # "relu" or "silu"
    head: nn.Module  # the NormalAffineTanhDistributionHead


def actor_layers(module: nn.Module) -> Optional[ActorLayers]:
    """The layers of a FeedForwardActor the kernels can run, or None: no input
    layer (or an nn.Identity), an MLPTorso of 1..4 Linear + ReLU/SiLU pairs
    without LayerNorm, every width a multiple of 16 up to 256, and a
    NormalAffineTanhDistributionHead with float bounds and 1..64 actions."""
    from stoix_amd.networks.base import FeedForwardActor
    from stoix_amd.networks.heads import NormalAffineTanhDistributionHead
    from stoix_amd.networks.torso import MLPTorso

    if type(module) is not FeedForwardActor or type(module.torso) is not MLPTorso:
        return None
    if module.input_layer is not None and type(module.input_layer) is not nn.Identity:
        return None
    head = module.action_head
    if type(head) is not NormalAffineTanhDistributionHead:
        return None
    if not all(isinstance(v, (int, float)) for v in (head.minimum, head.maximum, head.min_scale)):
        return None
    mods = list(module.torso.net)
    if len(mods) % 2 or not 1 <= len(mods) // 2 <= MAX_LAYERS:
        return None
    hidden, kinds = [], set()
    for lin, act in zip(mods[0::2], mods[1::2]):
        if type(lin) is not nn.Linear or lin.bias is None or act_kind(act) is None:
            return None
        if lin.out_features % 16 or lin.out_features > MAX_WIDTH:
            return None
        hidden.append(lin)
        kinds.add(act_kind(act))
    if len(kinds) != 1:
        return None
    for lin in (head.loc, head.scale):
        if type(lin) is not nn.Linear or lin.bias is None:
            return None
    if not 1 <= head.loc.out_features <= MAX_ACTION_DIM or head.scale.out_features != head.loc.out_features:
        return None
    return ActorLayers(hidden, kinds.pop(), head)


def actor_route_to_kernel(module: nn.Module, obs) -> bool:
    """True when ``module(obs)`` runs on the actor_mlp.hip kernels: knob on,
    extension built, no autocast, a non-empty 2-D fp32 CUDA observation that
    fits the first layer and needs no gradient, contiguous fp32 CUDA
    parameters, and a module ``actor_layers`` accepts."""
    if not actor_fused_enabled() or torch.is_autocast_enabled():
        return False
    if not isinstance(obs, torch.Tensor) or not obs.is_cuda or obs.dtype != torch.float32:
        return False
    if obs.dim() != 2 or obs.numel() == 0:
        return False
    if obs.requires_grad and torch.is_grad_enabled():
        return False
    layers = actor_layers(module)
    if layers is None or obs.shape[1] != layers.hidden[0].in_features:
        return False
    for lin in (*layers.hidden, layers.head.loc, layers.head.scale):
        for p in (lin.weight, lin.bias):
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                return False
    from stoix_amd import ops

    return ops.have_ext()


class _ActorMlpFn(torch.autograd.Function):
    """(loc, scale) [S, A] of the whole actor. ``params`` is W_1, b_1, ..,
    W_L, b_L, Wloc, bloc, Wscale, bscale. The forward keeps the scale's
    pre-softplus value and every H_l (for SiLU also Z_l) when a backward
    follows, else nothing. The observation takes no gradient."""

    @staticmethod
    def forward(ctx, obs, act, min_scale, save, *params):
        from stoix_amd.ops import ext

        ws, bs = list(params[0:-4:2]), list(params[1:-4:2])
        wloc, bloc, wscale, bscale = params[-4:]
        S, A = obs.shape[0], wloc.shape[0]
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=obs.device)
        loc, scale = new(S, A), new(S, A)
        spre = new(S, A) if save else new(0)
        hs = [new(S, w.shape[0]) for w in ws] if save else []
        zs = [new(S, w.shape[0]) for w in ws] if (save and act == "silu") else []
        if not ext(required=True).actor_mlp_fwd(
            obs, ws, bs, wloc, bloc, wscale, bscale, float(min_scale), ACT_CODES[act],
            loc, scale, spre, hs, zs,
        ):
            raise RuntimeError(f"actor_mlp_fwd does not take {tuple(obs.shape)} -> {[w.shape[0] for w in ws]} -> {A}")
        ctx.act, ctx.n_layers = act, len(ws)
        if save:
            ctx.save_for_backward(obs, spre, *params, *hs, *zs)
        return loc, scale

    @staticmethod
    @once_differentiable
    def backward(ctx, dloc, dscale):
        from stoix_amd.ops import ext

        kernels = ext(required=True)
        L, act = ctx.n_layers, ACT_CODES[ctx.act]
        obs, spre, *rest = ctx.saved_tensors
        params, saved = rest[: 2 * L + 4], rest[2 * L + 4 :]
        ws, bs = list(params[0:-4:2]), list(params[1:-4:2])
        wloc, bloc, wscale, bscale = params[-4:]
        hs = list(saved[:L])
        aux = hs if ctx.act == "relu" else list(saved[L:])
        S, A = spre.shape
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=obs.device)
        dzs, dzh = [new(S, w.shape[0]) for w in ws], new(2, S, A)
        if not kernels.actor_mlp_dgrad(
            dloc.contiguous(), dscale.contiguous(), spre, obs.shape[1], ws, bs,
            wloc, bloc, wscale, bscale, act, aux, dzs, dzh,
        ):
            raise RuntimeError(f"actor_mlp_dgrad does not take S={S}, A={A}")

        # dZ is formed, so the wgrad kernel applies no activation (code 0)
        none = new(0)
        need = ctx.needs_input_grad[4:]
        grads: List[Optional[Tensor]] = [None] * len(params)
        for l in range(L):
            if need[2 * l] or need[2 * l + 1]:
                dw, db = torch.empty_like(ws[l]), torch.empty_like(bs[l])
                x = obs if l == 0 else hs[l - 1]
                if not kernels.qens_linear_wgrad(dzs[l].unsqueeze(0), none, x, none, [dw], [db], 0):
                    raise RuntimeError(f"qens_linear_wgrad does not take S={S}, N={ws[l].shape[0]}, E=1")
                grads[2 * l], grads[2 * l + 1] = dw, db
        if any(need[2 * L :]):
            dws, dbs = [torch.empty_like(wloc), torch.empty_like(wscale)], [new(A), new(A)]
            if not kernels.qens_linear_wgrad(dzh, none, hs[L - 1], none, dws, dbs, 0):
                raise RuntimeError(f"qens_linear_wgrad does not take S={S}, N={A}, E=2")
            grads[2 * L :] = [dws[0], dbs[0], dws[1], dbs[1]]
        grads = [g if n else None for g, n in zip(grads, need)]
        return (None, None, None, None, *grads)


def actor_forward(module: nn.Module, obs: Tensor):
    """``module(obs)`` for a routed FeedForwardActor: the distribution the head
    builds, from the kernel's ``loc`` and ``scale``."""
    from stoix_amd.networks.distributions import AffineTanhTransformedDistribution

    layers = actor_layers(module)
    head = layers.head
    params = [p for lin in layers.hidden for p in (lin.weight, lin.bias)]
    params += [head.loc.weight, head.loc.bias, head.scale.weight, head.scale.bias]
    save = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    loc, scale = _ActorMlpFn.apply(obs.contiguous(), layers.act, head.min_scale, save, *params)
    return AffineTanhTransformedDistribution(loc, scale, head.minimum, head.maximum)
