"""Fused Q-ensemble critic MLP (ops/csrc/qens.hip): every dense layer of all
members of a ``MultiNetwork`` of obs-action critics in one launch, fp32 on
the matrix cores, with the obs/action concatenation, bias, ReLU/SiLU and their
backward inside the GEMM kernels.

``MultiNetwork.forward`` (networks/base.py) routes here when
``qens_route_to_kernel`` says so; every other case keeps its member loop. The
members' ``nn.Linear`` parameters stay where they are and are read in place.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from stoix_amd.ops.noisy import ACT_CODES, act_kind

Tensor = torch.Tensor

MAX_MEMBERS = 4


def qens_fused_enabled() -> bool:
    """STOIX_FUSED_QENS=0 keeps the member loop for eligible critic ensembles
    too. On by default: measured in one call, `bench.py --config sac` is 24.9%
    faster at 2048 envs and 62% faster at 512 (profiles/qens_SUMMARY.md)."""
    return os.environ.get("STOIX_FUSED_QENS", "1") == "1"


# One layer of the ensemble: the members' nn.Linear modules and the
# activation that follows ("relu", "silu" or None for the head).
Layer = Tuple[List[nn.Linear], Optional[str]]


def qens_layers(module: nn.Module) -> Optional[List[Layer]]:
    """The layers of a MultiNetwork the kernels can run, or None: 1..4
    FeedForwardCritic members with no input layer or an EmbeddingActionInput,
    an MLPTorso of Linear + ReLU/SiLU without LayerNorm and a
    ScalarCriticHead, all members of equal shapes."""
    from stoix_amd.networks.base import FeedForwardCritic
    from stoix_amd.networks.heads import ScalarCriticHead
    from stoix_amd.networks.inputs import EmbeddingActionInput
    from stoix_amd.networks.torso import MLPTorso

    nets = list(getattr(module, "networks", []))
    if not 1 <= len(nets) <= MAX_MEMBERS:
        return None
    per_member = []
    for net in nets:
        if type(net) is not FeedForwardCritic or type(net.torso) is not MLPTorso:
            return None
        if net.input_layer is not None and type(net.input_layer) is not EmbeddingActionInput:
            return None
        if type(net.critic_head) is not ScalarCriticHead:
            return None
        mods = list(net.torso.net)
        if len(mods) % 2:
            return None
        chain = []
        for lin, act in zip(mods[0::2], mods[1::2]):
            if type(lin) is not nn.Linear or lin.bias is None or act_kind(act) is None:
                return None
            chain.append((lin, act_kind(act)))
        chain.append((net.critic_head.linear, None))
        per_member.append(chain)
    first = per_member[0]
    for chain in per_member[1:]:
        if len(chain) != len(first):
            return None
        for (lin, act), (lin0, act0) in zip(chain, first):
            if act != act0 or lin.weight.shape != lin0.weight.shape:
                return None
    return [([chain[i][0] for chain in per_member], first[i][1]) for i in range(len(first))]


def _qens_tensor_eligible(is_cuda: bool, dtype: torch.dtype, dim: int, numel: int) -> bool:
    """The kernels take non-empty 2-D fp32 tensors on the GPU."""
    return is_cuda and dtype == torch.float32 and dim == 2 and numel > 0


def qens_route_to_kernel(module: nn.Module, inputs: Sequence) -> bool:
    """True when ``module(*inputs)`` runs on the qens.hip kernels: knob on,
    extension built, no autocast, fp32 CUDA tensors everywhere, 2-D inputs
    (obs, or obs and action) that fit the first layer, an observation that
    needs no gradient, and a module ``qens_layers`` accepts."""
    if not qens_fused_enabled() or torch.is_autocast_enabled():
        return False
    if len(inputs) not in (1, 2) or not all(isinstance(x, torch.Tensor) for x in inputs):
        return False
    for x in inputs:
        if not _qens_tensor_eligible(x.is_cuda, x.dtype, x.dim(), x.numel()):
            return False
    if inputs[0].requires_grad and torch.is_grad_enabled():
        return False
    if len(inputs) == 2 and inputs[0].shape[0] != inputs[1].shape[0]:
        return False
    layers = qens_layers(module)
    if layers is None:
        return False
    has_input_layer = module.networks[0].input_layer is not None
    if has_input_layer != (len(inputs) == 2):
        return False
    if sum(x.shape[1] for x in inputs) != layers[0][0][0].in_features:
        return False
    for lins, _ in layers:
        for lin in lins:
            for p in (lin.weight, lin.bias):
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                    return False
    from stoix_amd import ops

    return ops.have_ext()


class _QensLinearFn(torch.autograd.Function):
    """H [E, S, N] = act([x0 | x1] W_e^T + b_e) for the E members at once.

    ``x0`` is [S, K0] (shared by the members; takes no gradient) or the
    previous layer's [E, S, K0]; ``x1`` is None or the shared [S, K1]. The
    backward forms dZ = dH * act'(.) inside its kernels from the saved H
    (ReLU) or Z (SiLU), so nothing but H is handed between layers.
    """

    @staticmethod
    def forward(ctx, x0, x1, act, save, n_members, *params):
        from stoix_amd.ops import ext

        ws, bs = list(params[:n_members]), list(params[n_members:])
        S, N = x0.shape[-2], ws[0].shape[0]
        none = torch.empty(0, dtype=torch.float32, device=x0.device)
        h = torch.empty(n_members, S, N, dtype=torch.float32, device=x0.device)
        z = torch.empty_like(h) if (act == "silu" and save) else none
        if not ext(required=True).qens_linear_fwd(
            x0, none if x1 is None else x1, ws, bs, z, h, ACT_CODES[act]
        ):
            raise RuntimeError(f"qens_linear_fwd does not take {tuple(x0.shape)} -> {N}, E={n_members}")
        ctx.act, ctx.n_members = act, n_members
        if save:
            aux = h if act == "relu" else (z if act == "silu" else None)
            ctx.save_for_backward(x0, x1, aux, *ws)
        return h

    @staticmethod
    @once_differentiable
    def backward(ctx, dh):
        from stoix_amd.ops import ext

        x0, x1, aux, *ws = ctx.saved_tensors
        E, act = ctx.n_members, ACT_CODES[ctx.act]
        kernels = ext(required=True)
        dh = dh.contiguous()
        S, N = dh.shape[1], dh.shape[2]
        K0 = x0.shape[-1]
        none = torch.empty(0, dtype=torch.float32, device=dh.device)
        aux = none if aux is None else aux

        g_params = [None] * (2 * E)
        if any(ctx.needs_input_grad[5:]):
            dws = [torch.empty_like(w) for w in ws]
            dbs = [torch.empty(N, dtype=torch.float32, device=dh.device) for _ in ws]
            if not kernels.qens_linear_wgrad(dh, aux, x0, none if x1 is None else x1, dws, dbs, act):
                raise RuntimeError(f"qens_linear_wgrad does not take S={S}, N={N}, E={E}")
            g_params = [g if need else None for g, need in zip(dws + dbs, ctx.needs_input_grad[5:])]

        g_x0 = g_x1 = None
        if ctx.needs_input_grad[0]:
            if x0.dim() != 3:
                raise RuntimeError("the shared first input of a Q-ensemble layer takes no gradient")
            g_x0 = torch.empty(E, S, K0, dtype=torch.float32, device=dh.device)
            if not kernels.qens_linear_dgrad(dh, aux, ws, g_x0, 0, act, False):
                raise RuntimeError(f"qens_linear_dgrad does not take S={S}, N={N}, E={E}")
        if x1 is not None and ctx.needs_input_grad[1]:
            # the members' gradients of the shared action, summed in the kernel
            g_x1 = torch.empty(S, x1.shape[1], dtype=torch.float32, device=dh.device)
            if not kernels.qens_linear_dgrad(dh, aux, ws, g_x1, K0, act, True):
                raise RuntimeError(f"qens_linear_dgrad does not take S={S}, N={N}, E={E}")
        return (g_x0, g_x1, None, None, None, *g_params)


def qens_forward(module: nn.Module, inputs: Sequence[Tensor]) -> Tensor:
    """``module(*inputs)`` for a routed MultiNetwork: [E, S], one launch per
    layer, a view of the head's [E, S, 1]."""
    layers = qens_layers(module)
    x0 = inputs[0].contiguous()
    x1 = inputs[1].contiguous() if len(inputs) == 2 else None
    grad_on = torch.is_grad_enabled()
    needs = grad_on and x1 is not None and x1.requires_grad
    for lins, act in layers:
        ws = [lin.weight for lin in lins]
        bs = [lin.bias for lin in lins]
        save = needs or (grad_on and any(p.requires_grad for p in ws + bs))
        x0 = _QensLinearFn.apply(x0, x1, act, save, len(lins), *ws, *bs)
        needs, x1 = save, None
    return x0.squeeze(-1)
