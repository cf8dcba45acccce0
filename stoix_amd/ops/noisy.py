"""Fused NoisyLinear (ops/csrc/noisy.hip): forward, input gradient and
parameter gradients of the factorised-Gaussian noisy layer with the noisy
weight formed inside the GEMM kernels, and the in-place noise transform.

The layer (networks/layers.py) routes here when its tensors are on the GPU,
``STOIX_FUSED_NOISY=1`` is set, bf16 autocast is active and the shape is one the
kernels take; every other case keeps the torch path.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

Tensor = torch.Tensor

ACT_CODES = {None: 0, "silu": 1, "relu": 2}


def noisy_fused_enabled() -> bool:
    """STOIX_FUSED_NOISY=1 puts NoisyLinear on the noisy.hip kernels. Off by
    default: measured in one call on Rainbow/Snake, the fused path is 3.5%
    faster at 4096 envs and 4.0% slower at 1024 (profiles/noisy_linear_SUMMARY.md),
    and the default goes to the path that wins at both."""
    return os.environ.get("STOIX_FUSED_NOISY", "0") == "1"


def act_kind(module: Optional[nn.Module]) -> Optional[str]:
    """The activation a kernel epilogue can take over, or None."""
    if type(module) is nn.SiLU:
        return "silu"
    if type(module) is nn.ReLU:
        return "relu"
    return None


def _noisy_kernel_eligible(
    is_cuda: bool, dtype: torch.dtype, in_features: int, autocast_dtype: Optional[torch.dtype]
) -> bool:
    """The HIP path takes fp32/bf16 inputs on the GPU under bf16 autocast,
    with K a multiple of 8 (16-byte pieces of the fp32 parameters)."""
    if not noisy_fused_enabled() or not is_cuda:
        return False
    if autocast_dtype is not torch.bfloat16:
        return False
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    return in_features >= 8 and in_features % 8 == 0


def noisy_route_to_kernel(x: Tensor, layer: nn.Module) -> bool:
    autocast = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else None
    return (
        _noisy_kernel_eligible(
            x.is_cuda and layer.weight_mu.is_cuda, x.dtype, layer.in_features, autocast
        )
        and x.numel() > 0
        and x.shape[-1] == layer.in_features
        # the kernels read mu / sigma in 16-byte pieces
        and layer.weight_mu.is_contiguous()
        and layer.weight_sigma.is_contiguous()
        and layer.weight_mu.data_ptr() % 16 == 0
        and layer.weight_sigma.data_ptr() % 16 == 0
    )


def noise_transform_(flat: Tensor) -> Tensor:
    """f(x) = sign(x) sqrt(|x|) in place: one launch on the GPU, the same bits
    as the torch sequence it replaces."""
    if flat.is_cuda:
        from stoix_amd.ops import ext

        ext(required=True).noise_transform(flat)
    else:
        s = flat.sign()
        flat.abs_().sqrt_().mul_(s)
    return flat


def _aligned(t: Tensor) -> Tensor:
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _NoisyLinearFn(torch.autograd.Function):
    """out = act(x W^T + b) with W, b formed from (mu, sigma, eps) in the kernel.

    Returns ``(out, z)``: ``z`` is the bf16 pre-activation when an activation
    is fused and gradients are wanted, else None. A following layer may take
    ``z`` as its ``z_prev``: its input is then ``act_prev(z_prev)``, and its
    backward sends the gradient to ``z_prev`` (dgrad with the act' epilogue,
    ``bf16(dX * act'(z_prev))`` with dX still in fp32)
    and none to ``x``, so the activation's backward never runs on its own.
    """

    @staticmethod
    def forward(ctx, x, z_prev, mu_w, sigma_w, mu_b, sigma_b, eps_in, eps_out,
                act, act_prev, use_noise, save):
        from stoix_amd.ops import ext

        N, K = mu_w.shape
        x2 = _aligned(x.reshape(-1, K))
        S = x2.shape[0]
        none = torch.empty(0, dtype=torch.bfloat16, device=x.device)
        want_z = act is None or save
        z = torch.empty(S, N, dtype=torch.bfloat16, device=x.device) if want_z else none
        h = torch.empty(S, N, dtype=torch.bfloat16, device=x.device) if act else none
        ok = ext(required=True).noisy_linear_fwd(
            x2, mu_w, sigma_w, mu_b, sigma_b, eps_in, eps_out, z, h,
            ACT_CODES[act], bool(use_noise),
        )
        if not ok:
            raise RuntimeError(f"noisy_linear_fwd does not take S={S}, K={K}, N={N}")
        ctx.set_materialize_grads(False)
        ctx.act, ctx.act_prev, ctx.use_noise = act, act_prev, bool(use_noise)
        ctx.x_shape, ctx.x_dtype = x.shape, x.dtype
        if save:
            ctx.save_for_backward(x2, z_prev, mu_w, sigma_w, eps_in, eps_out, z if act else None)
        out_shape = (*x.shape[:-1], N)
        if act:
            return h.view(out_shape), (z if save else None)
        return z.view(out_shape), None

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_z):
        from stoix_amd.ops import ext

        x2, z_prev, mu_w, sigma_w, eps_in, eps_out, z = ctx.saved_tensors
        N, K = mu_w.shape
        S = x2.shape[0]
        dz = g_z
        if g_out is not None:
            dz_a = g_out.reshape(S, N)
            if ctx.act:  # the output went to a consumer that is not a fused layer
                zf = z.float()
                if ctx.act == "silu":
                    sg = torch.sigmoid(zf)
                    dact = sg * (1.0 + zf * (1.0 - sg))
                else:
                    dact = (zf > 0).float()
                dz_a = (dz_a.float() * dact).to(torch.bfloat16)
            dz = dz_a if dz is None else dz + dz_a
        if dz is None:
            return (None,) * 12
        dz = _aligned(dz.reshape(S, N))
        if dz.dtype not in (torch.float32, torch.bfloat16):
            dz = dz.float()
        kernels = ext(required=True)
        empty = torch.empty(0, dtype=torch.float32, device=dz.device)

        g_params = [None, None, None, None]
        if any(ctx.needs_input_grad[2:6]):
            dmu_w, dmu_b = torch.empty_like(mu_w), torch.empty(N, dtype=torch.float32, device=dz.device)
            dsg_w = torch.empty_like(mu_w) if ctx.use_noise else empty
            dsg_b = torch.empty_like(dmu_b) if ctx.use_noise else empty
            if not kernels.noisy_linear_wgrad(dz, x2, eps_in, eps_out, dmu_w, dsg_w, dmu_b, dsg_b):
                raise RuntimeError(f"noisy_linear_wgrad does not take S={S}, K={K}, N={N}")
            g_params = [dmu_w, dsg_w if ctx.use_noise else None, dmu_b, dsg_b if ctx.use_noise else None]
            g_params = [g if need else None for g, need in zip(g_params, ctx.needs_input_grad[2:6])]

        g_x = g_zprev = None
        through_prev = z_prev is not None and ctx.needs_input_grad[1]
        if through_prev or ctx.needs_input_grad[0]:
            out = torch.empty(S, K, dtype=torch.bfloat16, device=dz.device)
            zp = _aligned(z_prev.reshape(S, K)) if through_prev else torch.empty(
                0, dtype=torch.bfloat16, device=dz.device)
            ok = kernels.noisy_linear_dgrad(
                dz, mu_w, sigma_w, eps_in, eps_out, zp, out,
                ACT_CODES[ctx.act_prev] if through_prev else 0, ctx.use_noise,
            )
            if not ok:
                raise RuntimeError(f"noisy_linear_dgrad does not take S={S}, K={K}, N={N}")
            if through_prev:
                g_zprev = out.view(z_prev.shape)
            else:
                g_x = out.to(ctx.x_dtype).view(ctx.x_shape)
        return (g_x, g_zprev, *g_params, None, None, None, None, None, None)


def noisy_linear_fused(
    layer: nn.Module, x: Tensor, act: Optional[str] = None,
    pre: Optional[Tuple[Tensor, str]] = None,
) -> Tuple[Tensor, Optional[Tuple[Tensor, str]]]:
    """One fused NoisyLinear apply. ``pre`` is what the previous fused layer
    returned second: its pre-activation and activation kind, when ``x`` is
    that layer's output. Returns the output and this layer's own ``pre``."""
    z_prev, act_prev = pre if pre is not None else (None, None)
    save = torch.is_grad_enabled() and (
        x.requires_grad or any(p.requires_grad for p in layer.parameters(recurse=False))
    )
    out, z = _NoisyLinearFn.apply(
        x, z_prev, layer.weight_mu, layer.weight_sigma, layer.bias_mu, layer.bias_sigma,
        layer.eps_in, layer.eps_out, act, act_prev, layer.use_noise, save,
    )
    return out, ((z, act) if z is not None else None)
