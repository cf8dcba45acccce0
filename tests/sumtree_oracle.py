"""Oracles for the prioritised-replay sum-tree (buffers/per.py, ops/csrc/
per.hip), shared by tests/test_buffers.py (torch path, CPU) and
tests/test_sumtree_gpu.py (HIP kernels).

A tree here is the flat level-order float32 array of ``2 * cap`` entries:
root at 1, children of node k at 2k and 2k + 1, leaves at ``[cap, 2 cap)``.
"""
from __future__ import annotations

from typing import Dict, Iterator, Tuple

import torch

EPS32 = float(torch.finfo(torch.float32).eps)  # 2**-23
U_MAX = 1.0 - 2.0 ** -24  # the largest float32 below 1, which torch.rand can return

TREE_SIZES = (1, 2, 6, 1000, 2 ** 17 + 1)
UPDATE_BATCHES = (1, 63, 65, 1023, 1025, 8192, 8193)
SAMPLE_BATCHES = (1, 7, 64, 257)


def priorities(n_items: int, seed: int) -> torch.Tensor:
    """Float32 priorities in (0.01, 1.01) with ~30 % zeros scattered inside,
    a zero run in the middle and the last 2 % (at least the last item, when
    there are two or more) zero. Item 0 is kept positive."""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n_items, generator=g) + 0.01
    p[torch.rand(n_items, generator=g) < 0.3] = 0.0
    if n_items >= 2:
        p[n_items - max(1, n_items // 50):] = 0.0
    if n_items >= 100:
        p[n_items // 2: n_items // 2 + n_items // 20] = 0.0
    p[0] = 0.5
    return p


def update_batches(n_items: int, seed: int) -> Iterator[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
    """Successive update batches of every size in UPDATE_BATCHES: random
    indices (duplicates occur, always carrying identical priorities, because
    the priority is a function of the index within a batch) with zeros among
    the priorities. Yields ``(idx, prio, table)`` with ``prio = table[idx]``."""
    g = torch.Generator().manual_seed(seed)
    for b, n in enumerate(UPDATE_BATCHES):
        table = priorities(n_items, seed * 100 + b)
        idx = torch.randint(0, n_items, (n,), generator=g)
        if n >= 4:  # an adjacent duplicate pair as well as the random ones
            idx[1] = idx[0]
        yield idx, table[idx].contiguous(), table


def assert_tree_consistent(tree: torch.Tensor, cap: int, leaves: torch.Tensor, what: str) -> None:
    """The first ``len(leaves)`` leaves equal ``leaves`` bit for bit, the
    remaining leaves are 0, and every internal node is bit-equal to
    ``left + right`` evaluated in float32 on this very tree."""
    tree = tree.detach().cpu()
    assert tree.dtype == torch.float32 and tree.numel() == 2 * cap
    n = leaves.numel()
    assert torch.equal(tree[cap: cap + n], leaves), f"{what}: leaves differ from what was set"
    assert not tree[cap + n:].any(), f"{what}: a leaf beyond n_items was written"
    pairs = tree.view(cap, 2)
    sums = pairs[:, 0] + pairs[:, 1]  # float32: sums[k] = tree[2k] + tree[2k + 1]
    bad = (tree[1:cap] != sums[1:cap]).nonzero().flatten() + 1
    assert bad.numel() == 0, f"{what}: nodes {bad[:8].tolist()} are not left + right"


def adversarial_u(n: int, seed: int) -> Dict[str, torch.Tensor]:
    """Float32 draws ``u`` for a batch of n: uniform random, every stratum's
    lower end (0), every stratum's upper end (1 - 2**-24), and the two ends
    alternating in both phases."""
    g = torch.Generator().manual_seed(seed)
    lo = torch.zeros(n)
    hi = torch.full((n,), U_MAX)
    assert float(hi[0]) < 1.0
    even = torch.arange(n) % 2 == 0
    return {
        "random": torch.rand(n, generator=g),
        "zero": lo,
        "max": hi,
        "zero/max": torch.where(even, lo, hi),
        "max/zero": torch.where(even, hi, lo),
    }


def assert_draws_valid(tree: torch.Tensor, cap: int, depth: int, n_items: int,
                       u: torch.Tensor, out: torch.Tensor, what: str) -> float:
    """(b) every returned slot is < n_items and has priority > 0;
    (c) with c the exclusive float64 prefix sum of the float32 leaves and
    m_i = (i + u_i) * total32 / n in float64, the returned leaf j satisfies
    c_j - delta <= m_i <= c_{j+1} + delta, delta = (depth + 3) * EPS32 *
    total: a node of the tree carries one rounding per level below it, the
    walk subtracts at most one such node per level, and three roundings form
    the mass (total / n, i + u, the product). No draw is excluded. Returns
    the largest distance outside [c_j, c_{j+1}] in units of delta."""
    tree = tree.detach().cpu()
    out = out.detach().cpu()
    n = u.numel()
    assert out.shape == (n,) and out.dtype == torch.long
    leaves = tree[cap: cap + n_items]
    assert float(tree[1]) > 0, "the oracle needs a positive root"
    assert ((out >= 0) & (out < n_items)).all(), f"{what}: slot outside [0, n_items)"
    zero = (leaves[out] <= 0).nonzero().flatten()
    assert zero.numel() == 0, (
        f"{what}: draws {zero[:8].tolist()} returned zero-priority slots "
        f"{out[zero[:8]].tolist()} ({zero.numel()} of {n})")
    l64 = leaves.double()
    c = torch.cat([torch.zeros(1, dtype=torch.float64), l64.cumsum(0)])
    total = float(tree[1])
    m = (torch.arange(n, dtype=torch.float64) + u.double()) * total / n
    delta = (depth + 3) * EPS32 * total
    outside = torch.maximum(c[out] - m, m - c[out + 1]).clamp(min=0.0)
    worst = float(outside.max()) / delta
    assert worst <= 1.0, f"{what}: a draw lies {worst:.3f} delta outside its leaf's interval"
    return worst
