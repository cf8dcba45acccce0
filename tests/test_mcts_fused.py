"""The MCTS step functions on the CPU: the batched torch composition against
the scalar float32 oracle, bit for bit, and the STOIX_FUSED_MCTS switch."""
import pytest
import torch

from mcts_oracle import ARENA_FIELDS, C_PUCT, new_search, oracle_search
from stoix_amd import ops
from stoix_amd.search import mcts

SHAPES = [(5, 3, 12), (3, 2, 20), (4, 18, 9)]
MODES = ["bushy", "chain", "flat"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_torch_steps_match_scalar_oracle_bit_for_bit(shape, mode):
    B, A, S = shape
    arena, emb_arena, fn = new_search(B, A, S, mode)
    got = mcts._run_simulations(arena, emb_arena, fn, S, C_PUCT)
    want, depth = oracle_search(B, A, S, mode)
    for k in ARENA_FIELDS:
        assert torch.equal(getattr(got, k), want[k]), f"arena.{k} differs from the oracle"
    # the modes do what they are for
    assert torch.equal(got.visit[:, 0], torch.full((B,), S + 1.0))
    if mode == "chain":
        assert (depth.max(dim=1).values == S).all()
        assert torch.equal(got.parent[:, 1:], torch.arange(S).expand(B, S))
    if mode == "flat":
        assert (got.min_q == 0).all() and (got.max_q == 0).all()
    if mode == "bushy":
        assert (got.max_q > got.min_q).all()


def test_mcts_fused_enabled_honours_the_switch(monkeypatch):
    monkeypatch.delenv("STOIX_FUSED_MCTS", raising=False)
    assert mcts.mcts_fused_enabled()
    monkeypatch.setenv("STOIX_FUSED_MCTS", "0")
    assert not mcts.mcts_fused_enabled()
    monkeypatch.setenv("STOIX_FUSED_MCTS", "1")
    assert mcts.mcts_fused_enabled()


def test_cpu_search_never_asks_for_the_extension(monkeypatch):
    def no_ext(*args, **kwargs):
        raise AssertionError("the CPU search asked for the HIP extension")

    monkeypatch.setattr(ops, "ext", no_ext)
    monkeypatch.setenv("STOIX_FUSED_MCTS", "1")
    B, A, S = 3, 4, 5
    arena, emb_arena, fn = new_search(B, A, S, "bushy")
    mcts._run_simulations(arena, emb_arena, fn, S, C_PUCT)
    assert torch.equal(arena.visit[:, 0], torch.full((B,), S + 1.0))
    emb = {"h": torch.arange(B).unsqueeze(1)}
    out = mcts.mcts_search(
        torch.zeros(B, 2), emb, torch.zeros(B, A), torch.zeros(B), fn, S,
        dirichlet_alpha=None, temperature=0.0,
    )
    assert out.action.shape == (B,)
