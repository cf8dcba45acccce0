"""GPU tests of the MCTS kernels (ops/csrc/mcts.hip) against the torch step
functions on the same arena. Every comparison is exact: the search is a chain
of arg-maxes, so the kernels are held to bit-equality, step by step and over
whole searches."""
import pytest
import torch

from mcts_oracle import (C_PUCT, assert_arenas_equal, clone_arena, make_recurrent_fn,
                         make_root, new_search)
from stoix_amd import ops
from stoix_amd.search import mcts

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def ext():
    return ops.ext(required=True)


def _grown(B, A, S, mode, sims, monkeypatch):
    """An arena of S + 1 slots with ``sims`` simulations run by the torch path."""
    arena, emb_arena, fn = new_search(B, A, S, mode, DEV)
    monkeypatch.setenv("STOIX_FUSED_MCTS", "0")
    mcts._run_simulations(arena, emb_arena, fn, sims, C_PUCT)
    monkeypatch.delenv("STOIX_FUSED_MCTS")
    return arena, emb_arena, fn


@pytest.mark.parametrize("mode", ["bushy", "chain", "flat"])
@pytest.mark.parametrize("sims", [0, 1, 7])
def test_each_step_matches_torch_on_the_same_arena(sims, mode, monkeypatch):
    B, A, S = 37, 5, 8
    arena, emb_arena, fn = _grown(B, A, S, mode, sims, monkeypatch)
    sim = sims + 1
    before = clone_arena(arena)
    sp_t, sa_t = mcts._select_torch(arena, sim, C_PUCT)
    sp_k, sa_k = mcts._select_hip(arena, sim, C_PUCT)
    assert_arenas_equal(arena, before, "mcts_select_kernel wrote to the arena")
    assert torch.equal(sp_k, sp_t), "mcts_select_kernel: sel_parent"
    assert torch.equal(sa_k, sa_t), "mcts_select_kernel: sel_action"

    parent_emb = {k: v[arena.batch, sp_t] for k, v in emb_arena.items()}
    _, reward, discount, logits, value = fn(parent_emb, sa_t)
    prior_new = torch.softmax(logits, dim=-1)
    a_t, a_k = clone_arena(arena), clone_arena(arena)
    mcts._expand_backup_torch(a_t, sim, sp_t, sa_t, reward, discount, prior_new, value)
    mcts._expand_backup_hip(a_k, sim, sp_t, sa_t, reward, discount, prior_new, value)
    assert_arenas_equal(a_k, a_t, "mcts_expand_backup_kernel")


def _search(B, A, S, mode, fused, monkeypatch):
    monkeypatch.setenv("STOIX_FUSED_MCTS", "1" if fused else "0")
    arena, emb_arena, fn = new_search(B, A, S, mode, DEV)
    return mcts._run_simulations(arena, emb_arena, fn, S, C_PUCT)


WHOLE = [
    (1, 2, 1, "bushy"),
    (5, 3, 2, "bushy"),
    (67, 2, 33, "chain"),  # several trees per wave, ragged last wave, depth 33
    (130, 18, 16, "bushy"),  # A not a power of two, groups of 32
    (9, 70, 6, "bushy"),  # A > 64: lanes stride over the actions
    (64, 4, 24, "flat"),  # every score ties
]


@pytest.mark.parametrize("case", WHOLE, ids=lambda c: "x".join(map(str, c)))
def test_whole_search_matches_torch(case, monkeypatch):
    B, A, S, mode = case
    fused = _search(B, A, S, mode, True, monkeypatch)
    torch_ = _search(B, A, S, mode, False, monkeypatch)
    assert_arenas_equal(fused, torch_, f"search {case}")
    assert torch.equal(fused.visit[:, 0], torch.full((B,), S + 1.0, device=DEV))
    if mode == "chain":
        want = torch.arange(S, device=DEV).expand(B, S)
        assert torch.equal(fused.parent[:, 1:], want)


def _public(kind, fused, monkeypatch):
    monkeypatch.setenv("STOIX_FUSED_MCTS", "1" if fused else "0")
    B, A, S = 33, 6, 12
    emb, _, value = make_root(B, A, "bushy", DEV)
    gen = torch.Generator(device=DEV).manual_seed(11)
    torch.manual_seed(5)  # the Dirichlet noise draws from the default generator
    if kind == "discrete":
        logits = torch.log(make_root(B, A, "bushy", DEV)[1])
        return mcts.mcts_search(
            torch.zeros(B, 2, device=DEV), emb, logits, value, make_recurrent_fn(A, "bushy"), S,
            dirichlet_alpha=0.3, temperature=1.0, generator=gen,
        )
    base = make_recurrent_fn(A, "bushy")
    cands = torch.linspace(-1, 1, A, device=DEV).view(1, A, 1).repeat(B, 1, 1)

    def fn(embedding, action):  # the arm is recovered from the candidate value
        arm = ((action.squeeze(-1) + 1) * (A - 1) / 2).round().long()
        new_emb, reward, discount, _, v = base(embedding, arm)
        return new_emb, reward, discount, cands, v

    return mcts.sampled_mcts_search(
        torch.zeros(B, 2, device=DEV), emb, cands, value, fn, S, temperature=1.0, generator=gen,
    )


@pytest.mark.parametrize("kind", ["discrete", "sampled"])
def test_public_search_matches_torch_path(kind, monkeypatch):
    fused = _public(kind, True, monkeypatch)
    torch_ = _public(kind, False, monkeypatch)
    assert torch.equal(fused.action, torch_.action)
    assert torch.equal(fused.action_weights, torch_.action_weights)
    assert torch.equal(fused.search_value, torch_.search_value)
    assert float(fused.action_weights.sum()) == pytest.approx(fused.action.shape[0], rel=1e-5)


def test_fused_search_has_no_host_sync(monkeypatch):
    monkeypatch.setenv("STOIX_FUSED_MCTS", "1")
    B, A, S = 16, 4, 6
    emb, prior, value = make_root(B, A, "bushy", DEV)
    logits, obs = torch.log(prior), torch.zeros(B, 2, device=DEV)
    fn = make_recurrent_fn(A, "bushy")
    kw = dict(dirichlet_alpha=None, temperature=0.0)
    mcts.mcts_search(obs, emb, logits, value, fn, S, **kw)  # warm up: first-use set-up may sync
    torch.cuda.synchronize()
    flag = torch.ones(1, device=DEV)
    caught = False
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:  # the mode must catch a synchronisation for the test to mean anything
            bool(flag.any())
        except RuntimeError:
            caught = True
        if caught:
            out = mcts.mcts_search(obs, emb, logits, value, fn, S, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not caught:
        pytest.skip("this torch build does not implement sync debug mode 'error' on ROCm")
    assert out.action.shape == (B,)


def test_fused_search_is_deterministic(monkeypatch):
    a = _search(130, 18, 16, "bushy", True, monkeypatch)
    b = _search(130, 18, 16, "bushy", True, monkeypatch)
    assert_arenas_equal(a, b, "two fused runs")
