"""Batched array-based MCTS on device (the mctx replacement).

Functional parity with the mctx ``muzero_policy`` / ``gumbel_muzero_policy``
usage in the reference (/root/reference/stoix/systems/search/ff_az.py:377-379,
ff_mz.py): a fixed number of simulations over a preallocated node arena
([B, S+1] struct-of-arrays tensors), PUCT selection with min-max value
normalisation, expansion through a user ``recurrent_fn`` (real env step for
AlphaZero, learned dynamics for MuZero), and masked backward passes. Every
phase runs over all B trees simultaneously — the MI355X execution shape for
K16 of SURVEY.md §2.9.

One simulation is two steps around ``recurrent_fn``: ``_select`` (the PUCT
descent to an edge without a child) and ``_expand_backup`` (write the new
node, link it, back its value up to the root). On the GPU each step is one
kernel of ops/csrc/mcts.hip; on the CPU, or with STOIX_FUSED_MCTS=0, it is
the batched torch composition. The two are bit-equal and interchangeable on
the same arena, step by step.

``recurrent_fn(embedding, action) -> (embedding, reward, discount, prior_logits,
value)`` where ``embedding`` is a dict of [B, ...] tensors.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, NamedTuple, Optional, Tuple

import torch

from stoix_amd import ops

Tensor = torch.Tensor


class SearchOutput(NamedTuple):
    action: Tensor  # [B] chosen action
    action_weights: Tensor  # [B, A] normalised root visit counts
    search_value: Tensor  # [B] root value estimate


class _Arena:
    def __init__(self, B: int, N: int, A: int, device, value0: Tensor):
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=device)
        self.visit = z(B, N)
        self.value_sum = z(B, N)
        self.reward = z(B, N)
        self.discount = z(B, N)
        self.prior = z(B, N, A)
        self.children = torch.full((B, N, A), -1, dtype=torch.long, device=device)
        self.parent = torch.full((B, N), -1, dtype=torch.long, device=device)
        self.act_from_parent = z(B, N, dtype=torch.long)
        # min-max value normalisation bounds per tree
        self.min_q = torch.full((B,), 1e9, device=device)
        self.max_q = torch.full((B,), -1e9, device=device)
        self.batch = torch.arange(B, device=device)

    def q_value(self, nodes: Tensor) -> Tensor:
        v = self.visit[self.batch, nodes]
        return torch.where(v > 0, self.value_sum[self.batch, nodes] / v.clamp(min=1), torch.zeros_like(v))


def mcts_fused_enabled() -> bool:
    """STOIX_FUSED_MCTS=0 forces the torch step functions (A/B timing)."""
    return os.environ.get("STOIX_FUSED_MCTS", "1") != "0"


def _use_kernels(arena: _Arena) -> bool:
    return arena.visit.is_cuda and mcts_fused_enabled()


def _new_search(
    root_embedding: Dict[str, Tensor], root_prior: Tensor, root_value: Tensor, num_simulations: int
) -> Tuple[_Arena, Dict[str, Tensor]]:
    """Arena and embedding arena of ``num_simulations + 1`` slots with the
    root in slot 0, seeded with its prior row and its network value."""
    B, A = root_prior.shape
    N = num_simulations + 1
    device = root_prior.device
    arena = _Arena(B, N, A, device, root_value)
    arena.prior[:, 0] = root_prior
    arena.discount[:, 0] = 1.0

    # embedding arena: [B, N, ...] per field
    emb_arena = {
        k: torch.zeros((B, N, *v.shape[1:]), dtype=v.dtype, device=device)
        for k, v in root_embedding.items()
    }
    for k, v in root_embedding.items():
        emb_arena[k][:, 0] = v

    # seed the root with its network value
    arena.visit[:, 0] = 1.0
    arena.value_sum[:, 0] = root_value
    arena.min_q = torch.minimum(arena.min_q, root_value)
    arena.max_q = torch.maximum(arena.max_q, root_value)
    return arena, emb_arena


# ---------------------------------------------------------------- selection


def _select_torch(arena: _Arena, sim: int, c_puct: float) -> Tuple[Tensor, Tensor]:
    bidx = arena.batch
    B = bidx.shape[0]
    device = bidx.device
    # ---- selection: descend PUCT until a missing child edge
    node = torch.zeros(B, dtype=torch.long, device=device)
    descending = torch.ones(B, dtype=torch.bool, device=device)
    sel_parent = torch.zeros(B, dtype=torch.long, device=device)
    sel_action = torch.zeros(B, dtype=torch.long, device=device)
    for _ in range(sim):
        child_idx = arena.children[bidx, node]  # [B, A]
        child_visit = torch.where(
            child_idx >= 0, arena.visit[bidx.unsqueeze(1), child_idx.clamp(min=0)], torch.zeros_like(child_idx, dtype=torch.float32)
        )
        child_q = torch.where(
            child_idx >= 0,
            arena.value_sum[bidx.unsqueeze(1), child_idx.clamp(min=0)] / child_visit.clamp(min=1),
            torch.zeros_like(child_visit),
        )
        # child value from the parent's perspective: r + gamma*q, min-max normalised
        child_r = torch.where(
            child_idx >= 0, arena.reward[bidx.unsqueeze(1), child_idx.clamp(min=0)], torch.zeros_like(child_visit)
        )
        child_g = torch.where(
            child_idx >= 0, arena.discount[bidx.unsqueeze(1), child_idx.clamp(min=0)], torch.zeros_like(child_visit)
        )
        q_edge = child_r + child_g * child_q
        span = (arena.max_q - arena.min_q).clamp(min=1e-3).unsqueeze(1)
        # unvisited children score as the PARENT's normalised value
        # (mctx qtransform_by_parent_and_siblings): scoring them as the
        # global minimum lets one mediocre visited arm starve its
        # unvisited siblings for hundreds of simulations
        parent_q = (arena.q_value(node) - arena.min_q) / span.squeeze(1)
        q_norm = torch.where(
            child_visit > 0,
            (q_edge - arena.min_q.unsqueeze(1)) / span,
            parent_q.unsqueeze(1).expand_as(q_edge),
        )
        parent_visit = arena.visit[bidx, node].unsqueeze(1)
        ucb = q_norm + c_puct * arena.prior[bidx, node] * torch.sqrt(parent_visit.clamp(min=1)) / (
            1.0 + child_visit
        )
        best_a = ucb.argmax(dim=-1)
        has_child = child_idx.gather(1, best_a.unsqueeze(1)).squeeze(1) >= 0
        # record the (parent, action) where the descent stops
        stop_here = descending & ~has_child
        sel_parent = torch.where(stop_here, node, sel_parent)
        sel_action = torch.where(stop_here, best_a, sel_action)
        step_child = child_idx.gather(1, best_a.unsqueeze(1)).squeeze(1).clamp(min=0)
        node = torch.where(descending & has_child, step_child, node)
        descending = descending & has_child
    # trees still descending at max depth expand from their current node
    sel_parent = torch.where(descending, node, sel_parent)
    if bool(descending.any()):
        # pick their PUCT action at the final node (recompute quickly)
        child_idx = arena.children[bidx, node]
        ucb = arena.prior[bidx, node]
        best_a = ucb.argmax(dim=-1)
        sel_action = torch.where(descending, best_a, sel_action)
    return sel_parent, sel_action


def _select_hip(arena: _Arena, sim: int, c_puct: float) -> Tuple[Tensor, Tensor]:
    """mcts_select_kernel: no host involvement. At simulation ``sim`` the
    tree holds ``sim`` nodes, so a path has at most ``sim - 1`` child steps
    and the descent always ends at a missing edge."""
    sel_parent = torch.empty_like(arena.batch)
    sel_action = torch.empty_like(arena.batch)
    ops.ext(required=True).mcts_select(
        arena.visit, arena.value_sum, arena.reward, arena.discount, arena.prior,
        arena.children, arena.min_q, arena.max_q, float(c_puct), sel_parent, sel_action,
    )
    return sel_parent, sel_action


def _select(arena: _Arena, sim: int, c_puct: float) -> Tuple[Tensor, Tensor]:
    """(sel_parent [B], sel_action [B]): the edge simulation ``sim`` expands."""
    if _use_kernels(arena):
        return _select_hip(arena, sim, c_puct)
    return _select_torch(arena, sim, c_puct)


# ------------------------------------------------------- expansion + backup


def _expand_backup_torch(
    arena: _Arena, sim: int, sel_parent: Tensor, sel_action: Tensor,
    reward: Tensor, discount: Tensor, prior_new: Tensor, value: Tensor,
) -> None:
    bidx = arena.batch
    B = bidx.shape[0]
    device = bidx.device
    new_node = sim
    arena.reward[:, new_node] = reward
    arena.discount[:, new_node] = discount
    arena.prior[:, new_node] = prior_new
    arena.parent[:, new_node] = sel_parent
    arena.act_from_parent[:, new_node] = sel_action
    arena.children[bidx, sel_parent, sel_action] = new_node

    # ---- backward: propagate value to the root (masked walk)
    g = value.clone()
    cur = torch.full((B,), new_node, dtype=torch.long, device=device)
    alive = torch.ones(B, dtype=torch.bool, device=device)
    for _ in range(sim + 1):
        af = alive.to(torch.float32)
        arena.visit[bidx, cur] += af
        arena.value_sum[bidx, cur] += g * af
        q_here = arena.value_sum[bidx, cur] / arena.visit[bidx, cur].clamp(min=1)
        arena.min_q = torch.where(alive, torch.minimum(arena.min_q, q_here), arena.min_q)
        arena.max_q = torch.where(alive, torch.maximum(arena.max_q, q_here), arena.max_q)
        g = arena.reward[bidx, cur] + arena.discount[bidx, cur] * g
        nxt = arena.parent[bidx, cur]
        alive = alive & (nxt >= 0)
        cur = nxt.clamp(min=0)


def _expand_backup_hip(
    arena: _Arena, sim: int, sel_parent: Tensor, sel_action: Tensor,
    reward: Tensor, discount: Tensor, prior_new: Tensor, value: Tensor,
) -> None:
    """mcts_expand_backup_kernel. The per-tree rows are cast to the arena's
    f32 as the torch path's assignments into the arena do."""
    B = arena.batch.shape[0]
    f32 = lambda t: t.to(torch.float32).expand(B).contiguous()
    ops.ext(required=True).mcts_expand_backup(
        arena.visit, arena.value_sum, arena.reward, arena.discount, arena.prior,
        arena.children, arena.parent, arena.act_from_parent, arena.min_q, arena.max_q,
        sel_parent, sel_action, sim, f32(reward), f32(discount),
        prior_new.to(torch.float32).expand_as(arena.prior[:, 0]).contiguous(), f32(value),
    )


def _expand_backup(
    arena: _Arena, sim: int, sel_parent: Tensor, sel_action: Tensor,
    reward: Tensor, discount: Tensor, prior_new: Tensor, value: Tensor,
) -> None:
    """Write node ``sim`` under (sel_parent, sel_action) and back ``value``
    up to the root, in place."""
    step = _expand_backup_hip if _use_kernels(arena) else _expand_backup_torch
    step(arena, sim, sel_parent, sel_action, reward, discount, prior_new, value)


def _run_simulations(
    arena: _Arena,
    emb_arena: Dict[str, Tensor],
    recurrent_fn: Callable,
    num_simulations: int,
    c_puct: float,
    expand_extras: Optional[Tuple[Tensor, Tensor]] = None,
) -> _Arena:
    """The simulation loop of both searches; returns the finished arena.

    ``expand_extras`` is None for the discrete search, where ``recurrent_fn``
    takes the selected action and returns prior logits. The sampled search
    passes ``(cand, prior_row)``: the candidate arena [B, N, K, act_dim], from
    which the continuous action is gathered and into which ``recurrent_fn``'s
    new candidates go, and the constant [B, K] prior row of every new node.
    """
    bidx = arena.batch
    for sim in range(1, num_simulations + 1):
        sel_parent, sel_action = _select(arena, sim, c_puct)

        # ---- expansion: recurrent_fn on the selected (parent, action)
        parent_emb = {k: v[bidx, sel_parent] for k, v in emb_arena.items()}
        if expand_extras is None:
            new_emb, reward, discount, prior_logits, value = recurrent_fn(parent_emb, sel_action)
            prior_new = torch.softmax(prior_logits, dim=-1)
        else:
            cand, prior_new = expand_extras
            action_cont = cand[bidx, sel_parent, sel_action]  # [B, act_dim]
            new_emb, reward, discount, new_cand, value = recurrent_fn(parent_emb, action_cont)
            cand[:, sim] = new_cand
        for k, v in new_emb.items():
            emb_arena[k][:, sim] = v
        _expand_backup(arena, sim, sel_parent, sel_action, reward, discount, prior_new, value)
    return arena


def _read_out(
    arena: _Arena, temperature: float, generator: Optional[torch.Generator]
) -> Tuple[Tensor, Tensor, Tensor]:
    """(chosen root arm [B], normalised root visit counts [B, A], root value [B])."""
    bidx = arena.batch
    device = bidx.device
    root_children = arena.children[:, 0]  # [B, A]
    counts = torch.where(
        root_children >= 0,
        arena.visit[bidx.unsqueeze(1), root_children.clamp(min=0)],
        torch.zeros_like(root_children, dtype=torch.float32),
    )
    weights = counts / counts.sum(-1, keepdim=True).clamp(min=1e-9)
    search_value = arena.value_sum[:, 0] / arena.visit[:, 0].clamp(min=1)
    if temperature <= 0:
        arm = weights.argmax(dim=-1)
    else:
        logits = torch.log(weights.clamp(min=1e-9)) / temperature
        u = torch.rand(logits.shape, device=device, generator=generator)
        gnoise = -torch.log((-torch.log(u.clamp(min=1e-10))).clamp(min=1e-10))
        arm = (logits + gnoise).argmax(dim=-1)
    return arm, weights, search_value


def mcts_search(
    root_obs: Tensor,
    root_embedding: Dict[str, Tensor],
    root_prior_logits: Tensor,
    root_value: Tensor,
    recurrent_fn: Callable,
    num_simulations: int,
    c_puct: float = 1.25,
    dirichlet_alpha: Optional[float] = 0.3,
    dirichlet_fraction: float = 0.25,
    temperature: float = 1.0,
    generator: Optional[torch.Generator] = None,
    gumbel: bool = False,
) -> SearchOutput:
    device = root_obs.device
    B, A = root_prior_logits.shape

    prior = torch.softmax(root_prior_logits, dim=-1)
    if dirichlet_alpha is not None and dirichlet_fraction > 0:
        noise = torch._standard_gamma(
            torch.full((B, A), dirichlet_alpha, device=device)
        )
        noise = noise / noise.sum(-1, keepdim=True).clamp(min=1e-9)
        prior = (1 - dirichlet_fraction) * prior + dirichlet_fraction * noise
    arena, emb_arena = _new_search(root_embedding, prior, root_value, num_simulations)
    _run_simulations(arena, emb_arena, recurrent_fn, num_simulations, c_puct)
    action, weights, search_value = _read_out(arena, temperature, generator)
    return SearchOutput(action=action, action_weights=weights, search_value=search_value)


class SampledSearchOutput(NamedTuple):
    action: Tensor  # [B, act_dim] chosen continuous action
    sampled_actions: Tensor  # [B, K, act_dim] root candidate actions
    action_weights: Tensor  # [B, K] normalised root visit counts
    search_value: Tensor  # [B] root value estimate


def sampled_mcts_search(
    root_obs: Tensor,
    root_embedding: Dict[str, Tensor],
    root_candidates: Tensor,  # [B, K, act_dim] sampled from the root policy
    root_value: Tensor,
    recurrent_fn: Callable,
    num_simulations: int,
    c_puct: float = 1.25,
    temperature: float = 1.0,
    generator: Optional[torch.Generator] = None,
) -> SampledSearchOutput:
    """Sampled MCTS for continuous actions (parity surface: mctx's sampled
    policies as used by /root/reference/stoix/systems/search/ff_sampled_az.py
    and ff_sampled_mz.py).

    Each node holds K candidate actions drawn from the node's policy; the
    tree then searches over the K discrete arms. Because arms are i.i.d.
    samples from the current policy, the sampled prior over arms is uniform
    (the policy density is already represented by the sampling itself —
    the Sampled MuZero beta-correction cancels for beta = pi).

    ``recurrent_fn(embedding, action[B, act_dim]) ->
        (embedding, reward, discount, candidates[B, K, act_dim], value)``
    """
    device = root_obs.device
    B, K, act_dim = root_candidates.shape
    N = num_simulations + 1
    prior_row = torch.full((B, K), 1.0 / K, device=device)
    arena, emb_arena = _new_search(root_embedding, prior_row, root_value, num_simulations)
    cand = torch.zeros((B, N, K, act_dim), device=device)
    cand[:, 0] = root_candidates
    _run_simulations(
        arena, emb_arena, recurrent_fn, num_simulations, c_puct, expand_extras=(cand, prior_row)
    )
    arm, weights, search_value = _read_out(arena, temperature, generator)
    action = root_candidates[arena.batch, arm]
    return SampledSearchOutput(
        action=action,
        sampled_actions=root_candidates,
        action_weights=weights,
        search_value=search_value,
    )
