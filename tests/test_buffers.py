"""Replay buffer tests: item, trajectory, prioritised sum-tree."""
import torch

from stoix_amd.buffers import ItemBuffer, PrioritisedBuffer, TrajectoryBuffer
from stoix_amd.buffers.per import SumTree


def test_item_buffer_roundtrip():
    buf = ItemBuffer(capacity=100, seed=0)
    for i in range(5):
        buf.add({"x": torch.full((10, 3), float(i)), "a": torch.full((10,), i, dtype=torch.long)})
    assert buf.size == 50
    s = buf.sample(32)
    assert s["x"].shape == (32, 3)
    # field alignment preserved
    assert (s["x"][:, 0].long() == s["a"]).all()


def test_item_buffer_wraps():
    buf = ItemBuffer(capacity=16, seed=0)
    for i in range(4):
        buf.add({"x": torch.full((8,), float(i))})
    assert buf.size == 16
    s = buf.sample(64)
    # oldest items (0) have been overwritten
    assert (s["x"] >= 2.0).all()


def test_trajectory_buffer_windows_contiguous():
    buf = TrajectoryBuffer(add_batch_size=4, max_length_time_axis=64, sample_sequence_length=8, seed=0)
    t = 0
    for _ in range(6):
        block = torch.arange(t, t + 8, dtype=torch.float32).unsqueeze(0).expand(4, -1)
        buf.add({"t": block})
        t += 8
    s = buf.sample(16)
    seq = s["t"]
    assert seq.shape == (16, 8)
    diffs = seq[:, 1:] - seq[:, :-1]
    assert (diffs == 1).all(), "sampled windows must be time-contiguous"


def test_sum_tree_proportional():
    tree = SumTree(8)
    idx = torch.arange(8)
    prio = torch.tensor([0.0, 0.0, 1.0, 0.0, 3.0, 0.0, 0.0, 0.0])
    tree.set(idx, prio)
    assert abs(tree.total.item() - 4.0) < 1e-6
    g = torch.Generator().manual_seed(0)
    samples = tree.sample(4000, g)
    counts = torch.bincount(samples, minlength=8).float()
    assert counts[2] > 0 and counts[4] > 0
    assert counts[[0, 1, 3, 5, 6, 7]].sum() == 0
    ratio = counts[4] / counts[2]
    assert 2.0 < ratio < 4.5  # expect ~3


def test_sum_tree_update_changes_distribution():
    tree = SumTree(16)
    tree.set(torch.arange(16), torch.ones(16))
    tree.set(torch.tensor([5]), torch.tensor([100.0]))
    g = torch.Generator().manual_seed(1)
    s = tree.sample(1000, g)
    assert (s == 5).float().mean() > 0.7


def test_prioritised_buffer_sample_and_writeback():
    buf = PrioritisedBuffer(
        add_batch_size=2, max_length_time_axis=32, sample_sequence_length=4, seed=0
    )
    for i in range(4):
        buf.add({"x": torch.randn(2, 8, 3)})
    assert buf.can_sample
    s = buf.sample(8, importance_sampling_exponent=0.4)
    assert s["x"].shape == (8, 4, 3)
    assert (s["_weights"] <= 1.0 + 1e-6).all()
    buf.set_priorities(s["_slots"], torch.rand(8) * 5)
    s2 = buf.sample(8)
    assert s2["x"].shape == (8, 4, 3)


def test_trajectory_branch_free_wrap():
    """After wrapping, window starts must lie in the valid region behind
    the write pointer (branch-free formula: oldest = (ptr - filled) % t_max)."""
    buf = TrajectoryBuffer(add_batch_size=2, max_length_time_axis=16,
                           sample_sequence_length=4, seed=0)
    import torch as T

    for i in range(5):  # 5 adds of 6 steps = 30 > 16 -> wrapped
        buf.add({"x": T.full((2, 6, 1), float(i))})
    assert buf.t_filled == 16
    assert buf.t_ptr == 30 % 16
    out = buf.sample(64)
    assert out["x"].shape == (64, 4, 1)
    # windows must be monotone in write order: along the time axis the
    # values (add indices) never decrease by more than 0 (consecutive
    # windows span one or two adds)
    v = out["x"][..., 0]
    assert (v.diff(dim=1) >= 0).all()
    # and never include data older than the valid region (adds 0-1 were
    # overwritten: values 0 can survive only at slots not yet rewritten)
    # oldest surviving step is at (ptr - filled) % 16
    t0 = out["_t0"]
    assert ((t0 >= 0) & (t0 < 16)).all()


def test_prioritised_add_revalidates_block_boundary_windows():
    """Windows straddling an add-block boundary must become sampleable on
    the NEXT add (round-1 regression: slots invalidated behind the write
    head were never re-validated until the ring wrapped, starving half the
    data at small block sizes)."""
    buf = PrioritisedBuffer(
        add_batch_size=2, max_length_time_axis=32, sample_sequence_length=3,
        device="cpu", seed=0,
    )
    mk = lambda: {"x": torch.randn(2, 4, 1)}
    buf.add(mk())
    leaves = buf.tree.tree[buf.tree.capacity : buf.tree.capacity + buf.n_slots].view(2, 32)
    # after add 1 (cols 0-3): starts 0,1 valid; 2,3 would cross the head
    assert (leaves[:, 0:2] > 0).all() and (leaves[:, 2:4] == 0).all()
    buf.add(mk())
    leaves = buf.tree.tree[buf.tree.capacity : buf.tree.capacity + buf.n_slots].view(2, 32)
    # after add 2 (cols 4-7): the boundary starts 2,3 are re-validated,
    # 4,5 valid, 6,7 cross the new head
    assert (leaves[:, 0:6] > 0).all(), leaves[0, :10]
    assert (leaves[:, 6:8] == 0).all()
    # unwritten region stays unsampleable
    assert (leaves[:, 8:] == 0).all()


def test_sum_tree_random_ops_match_naive_reference():
    """Property test: arbitrary interleavings of batched set() calls keep
    the tree consistent with a naive array-of-priorities reference —
    root == sum, every internal node == sum of children, and stratified
    samples only land on positive-priority items."""
    from hypothesis import given, settings
    from hypothesis import strategies as st

    @settings(max_examples=30, deadline=None, derandomize=True)
    @given(
        st.lists(
            st.lists(
                st.tuples(st.integers(0, 99), st.floats(0.0, 10.0)),
                min_size=1, max_size=16,
            ),
            min_size=1, max_size=8,
        ),
        st.randoms(use_true_random=False),
    )
    def run(batches, rnd):
        tree = SumTree(100)
        ref = torch.zeros(100)
        for batch in batches:
            idx = torch.tensor([i for i, _ in batch], dtype=torch.long)
            pr = torch.tensor([p for _, p in batch])
            # duplicate indices: LAST write wins in the reference; the
            # tree's contract is "an arbitrary scatter winner among the
            # batch" — feed deduped batches to compare exactly
            seen = {}
            for i, p in batch:
                seen[i] = p
            idx = torch.tensor(list(seen.keys()), dtype=torch.long)
            pr = torch.tensor(list(seen.values()))
            tree.set(idx, pr)
            ref[idx] = pr
            # invariant: every internal node equals its children's sum
            t = tree.tree
            cap = tree.capacity
            torch.testing.assert_close(t[cap : cap + 100], ref, rtol=1e-5, atol=1e-5)
            for node in range(1, cap):
                torch.testing.assert_close(
                    t[node], t[2 * node] + t[2 * node + 1], rtol=1e-4, atol=1e-4
                )
            if float(ref.sum()) > 0:
                g = torch.Generator().manual_seed(rnd.randrange(2**31))
                s = tree.sample(64, g)
                assert (ref[s] > 0).all(), "sampled a zero-priority item"

    run()


def test_trajectory_windows_valid_under_random_adds_property():
    """Property test: after ANY sequence of variable-sized adds (wrapping the
    circular time axis arbitrarily), every sampled window is (a) contiguous
    in global time, (b) entirely inside the currently-valid region (the last
    t_filled written steps — never straddling the write pointer), and (c)
    period-aligned relative to the oldest valid step."""
    from hypothesis import given, settings
    from hypothesis import strategies as st

    from stoix_amd.buffers.trajectory import TrajectoryBuffer

    @settings(max_examples=20, deadline=None, derandomize=True)
    @given(st.integers(0, 10_000))
    def run(seed):
        g = torch.Generator().manual_seed(seed)
        rows, t_max, seq = 4, 16, 5
        period = int(torch.randint(1, 4, (1,), generator=g))
        buf = TrajectoryBuffer(rows, t_max, seq, device="cpu", seed=seed, period=period)
        glob = 0  # global step counter; cell value = row*10_000 + global_t
        for _ in range(int(torch.randint(3, 10, (1,), generator=g))):
            t_block = int(torch.randint(1, t_max, (1,), generator=g))
            vals = (
                torch.arange(rows).unsqueeze(1) * 10_000
                + (glob + torch.arange(t_block)).unsqueeze(0)
            ).float()
            buf.add({"x": vals})
            glob += t_block
            if not buf.can_sample:
                continue
            out = buf.sample(64)
            x = out["x"]  # [64, seq]
            row_id = (x[:, 0] // 10_000).long()
            gt = x - row_id.unsqueeze(1).float() * 10_000
            # (a) contiguity
            assert torch.all(gt[:, 1:] - gt[:, :-1] == 1.0), seed
            # row consistency across the window
            assert torch.all((x // 10_000) == row_id.unsqueeze(1)), seed
            # (b) inside the valid region
            oldest = glob - buf.t_filled
            assert torch.all(gt[:, 0] >= oldest), (seed, oldest, gt[:, 0])
            assert torch.all(gt[:, -1] <= glob - 1), seed
            # (c) period alignment of starts
            assert torch.all((gt[:, 0] - oldest) % period == 0), seed

    run()


# ------------------------------------------- guarded descent (adversarial u)


def _tree_with(n_items, seed):
    from sumtree_oracle import priorities

    tree = SumTree(n_items)
    prio = priorities(n_items, seed)
    tree.set(torch.arange(n_items), prio)
    return tree, prio


def test_sum_tree_descent_lands_on_positive_items_for_adversarial_u():
    """Properties (b) and (c) of tests/sumtree_oracle.py for the torch
    descent, with u at the ends of every stratum (0 and 1 - 2**-24, which
    torch.rand can return) as well as random, on trees with interior zero
    runs and a zero tail. The unguarded rule ``mass >= left`` returned a
    zero-priority slot from the last stratum at u = 1 - 2**-24 in about
    0.5 % of such draws; uniform random u never shows it."""
    from sumtree_oracle import (SAMPLE_BATCHES, TREE_SIZES, adversarial_u,
                                assert_draws_valid, assert_tree_consistent)

    worst = 0.0
    for n_items in TREE_SIZES + (100_000,):
        for seed in range(3):
            tree, prio = _tree_with(n_items, seed)
            assert_tree_consistent(tree.tree, tree.capacity, prio, f"n_items={n_items}")
            for n in SAMPLE_BATCHES + (200, 1000):
                for name, u in adversarial_u(n, seed).items():
                    out = tree.sample(n, u=u)
                    worst = max(worst, assert_draws_valid(
                        tree.tree, tree.capacity, tree.depth, n_items, u, out,
                        f"n_items={n_items} seed={seed} batch={n} u={name}"))
    print(f"largest distance outside the leaf interval: {worst:.4f} delta")


def test_sum_tree_sample_takes_the_given_u():
    tree, prio = _tree_with(1000, 0)
    u = torch.rand(64, generator=torch.Generator().manual_seed(5))
    a = tree.sample(64, u=u)
    assert torch.equal(a, tree.sample(64, u=u.double()))  # converted to float32
    # drawn from the generator when u is not given: same stream, same result
    b = tree.sample(64, torch.Generator().manual_seed(5))
    assert torch.equal(a, b)
    import pytest

    with pytest.raises(ValueError):
        tree.sample(64, u=u[:63])


def test_prioritised_buffer_never_samples_behind_the_write_head(monkeypatch):
    """The slots straight behind the write head have priority 0: a window
    starting there would cross the head. With u = 1 - 2**-24 the last
    stratum's mass can round up to the total, and the unguarded descent then
    ran right down to such a slot: its IS weight (1 / 1e-12) ** beta is the
    batch maximum, and after the normalisation every other row's weight is
    close to 0. Every window must lie in written data, contiguous in time,
    and every weight must stay positive."""
    from sumtree_oracle import U_MAX

    rows, t_max, seq, t_block = 2, 32, 4, 8
    hits = 0
    for seed in range(4):
        buf = PrioritisedBuffer(add_batch_size=rows, max_length_time_axis=t_max,
                                sample_sequence_length=seq, seed=seed)
        g = torch.Generator().manual_seed(seed)
        glob = 0
        for _ in range(2 + seed):  # the head ends inside the ring, or wraps
            # cell value = global time + 1; unwritten storage stays 0
            block = (glob + 1 + torch.arange(t_block)).float().expand(rows, -1)
            buf.add({"t": block.contiguous()})
            glob += t_block
        leaves = buf.tree.tree[buf.tree.capacity: buf.tree.capacity + buf.n_slots]
        live = (leaves > 0).nonzero().flatten()
        buf.set_priorities(live, torch.rand(live.numel(), generator=g) * 5)
        leaves = buf.tree.tree[buf.tree.capacity: buf.tree.capacity + buf.n_slots]
        head = buf.t_ptr
        behind = [(head - 1 - k) % t_max for k in range(seq - 1)]
        assert (leaves.view(rows, t_max)[:, behind] == 0).all()

        monkeypatch.setattr(torch, "rand", lambda n, device=None, generator=None:
                            torch.full((n,), U_MAX, device=device))
        for batch in range(1, 257):
            s = buf.sample(batch)
            w = s["t"]
            assert (w.min() >= 1) and (w.diff(dim=1) == 1).all(), (
                f"seed {seed} batch {batch}: a window crosses the write head: "
                f"slots {s['_slots'][(w.diff(dim=1) != 1).any(1) | (w.min(1).values < 1)].tolist()}")
            assert (leaves[s["_slots"]] > 0).all()
            assert float(s["_weights"].min()) > 0
            hits += 1
        monkeypatch.undo()
    assert hits == 4 * 256
