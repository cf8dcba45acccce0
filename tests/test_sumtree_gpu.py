"""GPU tests of the prioritised-replay sum-tree kernels (ops/csrc/per.hip).
Updates are held to bit-equality: with the CPU SumTree after the same calls,
and of every internal node with ``left + right`` in float32. Draws are fed a
chosen ``u`` and held to bit-equality with the torch descent on a CPU copy of
the tree, to "positive priority, < n_items" and to the float64 prefix-sum
oracle of tests/sumtree_oracle.py. Nothing here is statistical."""
import pytest
import torch

from stoix_amd import ops
from stoix_amd.buffers.per import SumTree
from sumtree_oracle import (SAMPLE_BATCHES, TREE_SIZES, adversarial_u, assert_draws_valid,
                            assert_tree_consistent, priorities, update_batches)

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def ext():
    return ops.ext(required=True)


@pytest.mark.parametrize("n_items", TREE_SIZES)
def test_update_is_bit_equal_to_the_cpu_tree(n_items):
    """Depth 0, non-powers of two and a deep tree; batch sizes on both sides
    of every thread-count rounding and of the single-workgroup / multi-launch
    switch (8192 / 8193); successive batches with zeros and with duplicate
    indices that carry identical priorities."""
    cpu, gpu = SumTree(n_items, "cpu"), SumTree(n_items, DEV)
    assert (gpu.capacity, gpu.depth) == (cpu.capacity, cpu.depth)
    leaves = torch.zeros(n_items)
    for idx, prio, table in update_batches(n_items, seed=n_items):
        what = f"n_items={n_items} batch={idx.numel()}"
        cpu.set(idx, prio)
        gpu.set(idx.to(DEV), prio.to(DEV))
        touched = torch.zeros(n_items, dtype=torch.bool)
        touched[idx] = True
        # what was set is there, what was not touched is unchanged
        leaves = torch.where(touched, table, leaves)
        got = gpu.tree.cpu()
        assert_tree_consistent(got, gpu.capacity, leaves, what)
        assert torch.equal(got, cpu.tree), f"{what}: differs from the CPU tree"


@pytest.mark.parametrize("n_items", TREE_SIZES)
def test_sample_matches_torch_descent_and_oracle(ext, n_items):
    """Random u, every stratum's two ends (0 and 1 - 2**-24), batch sizes
    below, at and above a wave and a block; trees with ~30 % zero leaves, a
    zero run inside and a zero tail."""
    worst = 0.0
    for seed in range(2):
        prio = priorities(n_items, seed)
        cpu, gpu = SumTree(n_items, "cpu"), SumTree(n_items, DEV)
        gpu.set(torch.arange(n_items, device=DEV), prio.to(DEV))
        cpu.tree.copy_(gpu.tree.cpu())  # the torch descent walks the same tree
        assert_tree_consistent(cpu.tree, cpu.capacity, prio, f"n_items={n_items}")
        for n in SAMPLE_BATCHES:
            for name, u in adversarial_u(n, seed).items():
                what = f"n_items={n_items} seed={seed} batch={n} u={name}"
                out = torch.full((n,), -1, dtype=torch.long, device=DEV)
                ext.sumtree_sample(gpu.tree, u.to(DEV), out, gpu.capacity, gpu.depth, n_items)
                out = out.cpu()
                # (b), (c): no draw excluded
                worst = max(worst, assert_draws_valid(cpu.tree, cpu.capacity, cpu.depth,
                                                      n_items, u, out, what))
                # (a) bit-equal to the torch descent
                assert torch.equal(out, cpu.sample(n, u=u)), f"{what}: differs from torch"
                # and SumTree.sample hands u to the kernel unchanged
                assert torch.equal(gpu.sample(n, u=u.to(DEV)).cpu(), out), what
    print(f"n_items={n_items}: largest distance outside the leaf interval {worst:.4f} delta")


def test_bindings_refuse_inconsistent_arguments(ext):
    tree = SumTree(6, DEV)  # cap 8, depth 3
    tree.set(torch.arange(6, device=DEV), torch.ones(6, device=DEV))
    idx = torch.arange(4, device=DEV)
    prio = torch.ones(4, device=DEV)
    u = torch.zeros(4, device=DEV)
    out = torch.zeros(4, dtype=torch.long, device=DEV)
    ext.sumtree_update(tree.tree, idx, prio, 8, 3)
    ext.sumtree_sample(tree.tree, u, out, 8, 3, 6)
    bad_update = [
        (tree.tree[:8], idx, prio, 8, 3),  # tree.numel() != 2 * cap
        (tree.tree, idx, prio, 8, 4),  # cap != 1 << depth
        (tree.tree, idx, prio, 4, 2),  # tree.numel() != 2 * cap
        (tree.tree, idx, prio[:3], 8, 3),  # prio.numel() != idx.numel()
        (tree.tree, idx.int(), prio, 8, 3),
        (tree.tree.cpu(), idx, prio, 8, 3),
    ]
    for args in bad_update:
        with pytest.raises(RuntimeError):
            ext.sumtree_update(*args)
    bad_sample = [
        (tree.tree[:8], u, out, 8, 3, 6),
        (tree.tree, u, out, 8, 2, 6),
        (tree.tree, u, out, 8, 3, 9),  # n_items > cap
        (tree.tree, u, out, 8, 3, 0),
        (tree.tree, u, out[:3], 8, 3, 6),  # out.numel() != u.numel()
        (tree.tree, u.double(), out, 8, 3, 6),
        (tree.tree, u, out.int(), 8, 3, 6),
    ]
    for args in bad_sample:
        with pytest.raises(RuntimeError):
            ext.sumtree_sample(*args)
    torch.cuda.synchronize()
    assert torch.equal(tree.tree.cpu()[8:14], torch.ones(6))
