"""The optimiser tail of the replay learners: global-norm clip, Adam and the
polyak target update of up to four chains in two HIP launches
(ops/csrc/multi_adam.hip).

A chain is one ``torch.optim.Adam``, its parameters, an optional clip norm and
an optional polyak target. The kernels work on the tensors torch's optimiser
owns (``p``, ``p.grad``, ``state["exp_avg"]``, ``state["exp_avg_sq"]``,
``state["step"]``), so ``state_dict`` / ``load_state_dict``, an lr schedule
that rewrites ``param_groups`` and a switch back to the torch calls at any
step need no conversion. The one visible difference from the torch calls:
``p.grad`` is read, not rescaled in place by the clip.

``OptimTail.step`` runs the torch calls it replaces (``clip_grad_norm_``,
``opt.step()``, ``polyak_update``, in that order) with ``STOIX_FUSED_OPTIM=0``
(the default is ``1``) and whenever the call is ineligible: CPU tensors, a non-capturable optimiser
(its ``step`` lives on the host), weight decay, amsgrad, maximize, several
param groups, a tensor that is not contiguous fp32, more than 64 tensors or
more than 4096 chunks of 2048 elements in a chain.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence

import torch
import torch.nn as nn

Tensor = torch.Tensor

MAX_CHAINS = 4
MAX_CHUNKS = 4096  # per chain, of 2048 elements
_NO_STATE = {"exp_avg": None, "exp_avg_sq": None, "step": None}


def fused_optim_enabled() -> bool:
    """STOIX_FUSED_OPTIM=0 keeps the torch calls for eligible tails too. On by
    default: measured in one call, `bench.py --config sac` is 49% faster at
    2048 envs and 46% at 512, `--config rainbow` 12% at 4096 envs and 15% at
    1024 (profiles/optim_tail_multi_SUMMARY.md)."""
    return os.environ.get("STOIX_FUSED_OPTIM", "1") == "1"


@dataclass
class OptimChain:
    opt: torch.optim.Optimizer
    params: Iterable[Tensor]
    max_norm: Optional[float] = None  # None: no clip
    target: Optional[Iterable[Tensor]] = None  # polyak target parameters
    tau: float = 0.0

    def __post_init__(self):
        self.params = list(self.params)
        self.max_norm = None if self.max_norm is None else float(self.max_norm)
        if self.target is not None:
            self.target = list(self.target)
            assert len(self.target) == len(self.params), "one target per parameter"


def _adam_hyper(chain: OptimChain):
    """(hyper row, lr tensor or None) of an eligible chain, else None."""
    opt = chain.opt
    if type(opt) is not torch.optim.Adam or len(opt.param_groups) != 1:
        return None
    g = opt.param_groups[0]
    b1, b2 = g["betas"]
    if (not g.get("capturable") or g.get("weight_decay") or g.get("amsgrad")
            or g.get("maximize") or g.get("differentiable")
            or not isinstance(b1, float) or not isinstance(b2, float)):
        return None
    lr = g["lr"]
    lr_t = lr if torch.is_tensor(lr) else None
    clip = chain.max_norm is not None
    row = [b1, b2, float(g["eps"]), 0.0 if lr_t is not None else float(lr),
           chain.max_norm if clip else 0.0, float(clip), float(chain.tau)]
    return row, lr_t


def _adam_state(opt: torch.optim.Optimizer, p: Tensor) -> dict:
    """The parameter's Adam state, created as the capturable path of
    ``Adam._init_group`` creates it."""
    st = opt.state[p]
    if len(st) == 0:
        scalar = torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32
        st["step"] = torch.zeros((), dtype=scalar, device=p.device)
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
    return st


class OptimTail:
    """``step(active=None)`` replaces the ``clip_grad_norm_`` + ``opt.step()``
    + ``polyak_update`` lines of a learner. ``active[i] = False`` (TD3's
    delayed actor) leaves chain ``i``'s step, moments, parameters and target
    untouched. Returns True when the HIP kernels ran, False after the torch
    calls."""

    def __init__(self, chains: Sequence[OptimChain]):
        self.chains: List[OptimChain] = list(chains)
        self._partials: Optional[Tensor] = None

    # ------------------------------------------------------------ torch path

    def _torch_step(self, active: Sequence[bool]) -> None:
        from stoix_amd.parallel.dist import polyak_update

        for ch in self.chains:
            if ch.max_norm is not None:
                nn.utils.clip_grad_norm_(ch.params, ch.max_norm)
        for ch, on in zip(self.chains, active):
            if on:
                ch.opt.step()
        with torch.no_grad():
            for ch, on in zip(self.chains, active):
                if on and ch.target is not None:
                    polyak_update(ch.params, ch.target, ch.tau)

    # ------------------------------------------------------------- HIP path

    def _fused_step(self, active: Sequence[bool]) -> bool:
        chains = [ch for ch, on in zip(self.chains, active) if on]
        if len(chains) > MAX_CHAINS:
            return False
        params, grads, ms, vs, steps, tgts, chain_of, hyper, lrs = ([] for _ in range(9))
        for c, ch in enumerate(chains):
            row = _adam_hyper(ch)
            if row is None or not all(p.is_cuda for p in ch.params):
                return False
            hyper.append(row[0])
            lrs.append(row[1])
            targets = ch.target if ch.target is not None else [None] * len(ch.params)
            for p, tg in zip(ch.params, targets):
                g = p.grad
                if g is None and tg is None:  # torch skips it too
                    continue
                # without a gradient only the polyak of its target runs
                st = _adam_state(ch.opt, p) if g is not None else _NO_STATE
                params.append(p)
                grads.append(g)
                ms.append(st["exp_avg"])
                vs.append(st["exp_avg_sq"])
                steps.append(st["step"])
                tgts.append(tg)
                chain_of.append(c)
        if not params:
            return True
        if self._partials is None or self._partials.device != params[0].device:
            self._partials = torch.empty(MAX_CHAINS * MAX_CHUNKS, device=params[0].device)
        from stoix_amd import ops

        ext = ops.ext(required=True)
        args = (params, grads, ms, vs, steps, tgts, chain_of, hyper, lrs, self._partials)
        with torch.no_grad():
            if not ext.multi_adam_norm(*args):
                return False
            if not ext.multi_adam_update(*args):
                raise RuntimeError("multi_adam: launch B refused what launch A took")
        return True

    def step(self, active: Optional[Sequence[bool]] = None) -> bool:
        active = [True] * len(self.chains) if active is None else [bool(a) for a in active]
        assert len(active) == len(self.chains), "one active flag per chain"
        if fused_optim_enabled() and self._fused_step(active):
            return True
        self._torch_step(active)
        return False
