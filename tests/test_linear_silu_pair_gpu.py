"""GPU tests for linear_silu_pair (stoix_amd/ops/csrc/mlp.hip): both nets'
layer-1 Linear+SiLU forward in one launch, stored row-contiguous through an
LDS re-layout. The contract is bit-equality with two linear_silu calls, the
kernel it replaces in the fused PPO engine (STOIX_FUSED_L1), plus the
engine-level check that neither STOIX_FUSED_L1 nor STOIX_FUSED_TAIL changes
a parameter."""
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

ROW_TILE = 128  # rows per workgroup of the paired kernel (LSF_BM in mlp.hip)


@pytest.fixture(scope="module")
def ext():
    from stoix_amd import ops

    e = ops.ext(required=True)
    assert e is not None
    return e


@functools.lru_cache(maxsize=None)
def _operands(S, K, N):
    """Seeded operands that differ per net, one shared X. Never written to."""
    g = torch.Generator().manual_seed(9100 + 7 * S + 3 * K + N)
    X = torch.randn(S, K, generator=g).bfloat16().cuda()
    W = [(torch.randn(N, K, generator=g) * 0.3).bfloat16().cuda() for _ in range(2)]
    b = [torch.randn(N, generator=g).cuda() for _ in range(2)]
    return X, W, b


@functools.lru_cache(maxsize=None)
def _reference(S, K, N):
    """(Z, H) per net from the old kernel, computed once per shape."""
    from stoix_amd import ops

    e = ops.ext(required=True)
    X, W, b = _operands(S, K, N)
    out = []
    for i in range(2):
        Z = torch.empty(S, N, dtype=torch.bfloat16, device="cuda")
        H = torch.empty_like(Z)
        e.linear_silu(X, W[i], b[i], Z, H, 1)
        out.append((Z, H))
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.view(torch.int16)


@requires_gpu
@pytest.mark.parametrize("S", [ROW_TILE, 3 * ROW_TILE])
@pytest.mark.parametrize("K", [32, 64, 96])
@pytest.mark.parametrize("N", [128, 256, 512])
def test_pair_is_bit_equal_to_two_calls(ext, S, K, N):
    X, W, b = _operands(S, K, N)
    ref = _reference(S, K, N)
    out = [torch.zeros(S, N, dtype=torch.bfloat16, device="cuda") for _ in range(4)]
    assert ext.linear_silu_pair(X, W[0], b[0], out[0], out[1],
                                W[1], b[1], out[2], out[3]) is True
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(_bits(out[2 * i]), _bits(ref[i][0])), f"Z of net {i}"
        assert torch.equal(_bits(out[2 * i + 1]), _bits(ref[i][1])), f"H of net {i}"
    # the nets are not mixed up: their results differ
    assert not torch.equal(_bits(out[0]), _bits(out[2]))


@requires_gpu
def test_pair_into_stacked_buffers(ext):
    """Z_a/Z_c and H_a/H_c as the halves of [2, S, N] buffers, as the engine
    passes them."""
    S, K, N = 3 * ROW_TILE, 32, 256
    X, W, b = _operands(S, K, N)
    ref = _reference(S, K, N)
    Z = torch.zeros(2, S, N, dtype=torch.bfloat16, device="cuda")
    H = torch.zeros(2, S, N, dtype=torch.bfloat16, device="cuda")
    assert ext.linear_silu_pair(X, W[0], b[0], Z[0], H[0], W[1], b[1], Z[1], H[1])
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(_bits(Z[i]), _bits(ref[i][0]))
        assert torch.equal(_bits(H[i]), _bits(ref[i][1]))


@requires_gpu
def test_pair_overwrites_all_and_nothing_else(ext):
    """Outputs pre-filled with NaN between guard rows: every element is
    overwritten, no guard row is touched."""
    S, K, N = 3 * ROW_TILE, 64, 256
    G = 8  # guard rows on each side
    X, W, b = _operands(S, K, N)
    ref = _reference(S, K, N)
    GUARD = 3.0
    bufs = []
    for _ in range(4):
        t = torch.full((G + S + G, N), GUARD, dtype=torch.bfloat16, device="cuda")
        t[G:G + S] = float("nan")
        bufs.append(t)
    o = [t[G:G + S] for t in bufs]
    assert ext.linear_silu_pair(X, W[0], b[0], o[0], o[1], W[1], b[1], o[2], o[3])
    torch.cuda.synchronize()
    for j, t in enumerate(bufs):
        assert (t[:G] == GUARD).all() and (t[G + S:] == GUARD).all(), f"guard of output {j}"
        assert not torch.isnan(t[G:G + S]).any(), f"output {j} not fully written"
        assert torch.equal(_bits(t[G:G + S]), _bits(ref[j // 2][j % 2]))


@requires_gpu
def test_pair_rejections(ext):
    z = lambda *s, dtype=torch.bfloat16: torch.zeros(*s, dtype=dtype, device="cuda")
    S, K, N = ROW_TILE, 32, 128

    def call(X=None, W=None, b=None, O=None):
        X = z(S, K) if X is None else X
        W = z(N, K) if W is None else W
        b = z(N, dtype=torch.float32) if b is None else b
        O = z(S, N) if O is None else O
        return ext.linear_silu_pair(X, W, b, O, z(S, N), z(N, K),
                                    z(N, dtype=torch.float32), z(S, N), z(S, N))

    with pytest.raises(RuntimeError, match="dtype"):
        call(X=z(S, K).float())
    with pytest.raises(RuntimeError, match="contiguous"):
        call(X=z(K, S).t())
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ext.linear_silu_pair(z(S, 48), z(N, 48), z(N, dtype=torch.float32), z(S, N),
                             z(S, N), z(N, 48), z(N, dtype=torch.float32), z(S, N),
                             z(S, N))
    with pytest.raises(RuntimeError, match="weight shapes"):
        call(W=z(N + 128, K))
    with pytest.raises(RuntimeError, match="S \\* N"):
        call(O=z(S + 1, N))


# ------------------------------------------------------------------ engine


def _learner(l1, tail, num_envs=64, T=8, n_mb=2):
    """A small fused PPO learner (27 obs / 8 act Ant, H = 256) built with the
    two knobs set; they are read in the engine's constructor."""
    from stoix_amd import envs as environments
    from stoix_amd.config import compose
    from stoix_amd.systems.ppo.ff_ppo import PPOLearner
    from stoix_amd.utils.total_timestep_checker import check_total_timesteps

    cfg = compose(
        "default/anakin/default_ff_ppo_continuous.yaml",
        ["env=brax/ant", f"arch.total_num_envs={num_envs}",
         "arch.total_timesteps=null", "arch.num_updates=4",
         "arch.num_evaluation=1", "arch.seed=11",
         f"system.rollout_length={T}", f"system.num_minibatches={n_mb}",
         "system.epochs=1", "logger.loggers=[]", "system.compute_dtype=bf16"],
    )
    cfg.arch.n_devices = 1
    check_total_timesteps(cfg)
    device = torch.device("cuda:0")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("STOIX_FUSED_L1", l1)
        mp.setenv("STOIX_FUSED_TAIL", tail)
        torch.manual_seed(11)
        env = environments.make_single(cfg, num_envs, device, seed=3)
        learner = PPOLearner(cfg, env, device)
    F_ = learner.fused
    assert F_ is not None
    assert F_.fused_l1 == (l1 != "0") and F_.fused_tail == (tail != "0")
    assert F_._tail_eligible() == (tail != "0")
    return learner


@requires_gpu
def test_engine_helper_and_fallback(ext):
    """The engine's layer-1 helper gives the same Z1/H1 with the knob on and
    off. For a shape the pair rejects (64 rows, no multiple of the row tile)
    the pair reports False with nothing launched and the helper lands on the
    old path: linear_silu shares the 128-row tile, so the old path is
    recognised by its own tile error, not by a silent pad."""
    on, off = _learner("1", "1"), _learner("0", "1")
    Fon, Foff = on.fused, off.fused
    S, K1P, H = Fon.S, Fon.K1P, Fon.H
    assert S % ROW_TILE == 0
    g = torch.Generator().manual_seed(5)
    X = torch.randn(S, K1P, generator=g).bfloat16().cuda()
    Fon.layer1_forward(X)
    Foff.layer1_forward(X)
    torch.cuda.synchronize()
    assert torch.equal(_bits(Fon.Z1), _bits(Foff.Z1))
    assert torch.equal(_bits(Fon.H1), _bits(Foff.H1))
    assert Fon.Z1.float().abs().sum().item() > 0
    bad = X[:64].contiguous()
    ac, cc = Fon.actor_chain, Fon.critic_chain
    Zs = torch.full((2, 64, H), 7.0, dtype=torch.bfloat16, device="cuda")
    Hs = torch.full((2, 64, H), 7.0, dtype=torch.bfloat16, device="cuda")
    assert ext.linear_silu_pair(
        bad, ac.views16["W1"], ac.views["b1"], Zs[0], Hs[0],
        cc.views16["W1"], cc.views["b1"], Zs[1], Hs[1]) is False
    torch.cuda.synchronize()
    assert (Zs == 7.0).all() and (Hs == 7.0).all()
    Fon.Z1, Fon.H1 = Zs, Hs
    with pytest.raises(RuntimeError, match="linear_silu tile constraints"):
        Fon.layer1_forward(bad)


@requires_gpu
def test_pair_rejects_width_without_writing(ext):
    """N not a multiple of the 128-column tile: False, outputs untouched."""
    z = lambda *s, dtype=torch.bfloat16: torch.full(s, 7.0, dtype=dtype, device="cuda")
    S, K, N = ROW_TILE, 32, 192
    out = [z(S, N) for _ in range(4)]
    assert ext.linear_silu_pair(z(S, K), z(N, K), z(N, dtype=torch.float32), out[0],
                                out[1], z(N, K), z(N, dtype=torch.float32), out[2],
                                out[3]) is False
    torch.cuda.synchronize()
    assert all((o == 7.0).all() for o in out)


@requires_gpu
def test_knobs_do_not_change_an_update_step():
    """64 envs, T = 8, 2 minibatches: after one update_step from the same
    seed every parameter is equal across the four knob combinations."""
    snaps = {}
    for l1, tail in itertools.product("01", "01"):
        learner = _learner(l1, tail)
        learner.update_step()
        torch.cuda.synchronize()
        snaps[(l1, tail)] = learner.snapshot_params()
        del learner
    base = snaps[("0", "0")]
    n = 0
    for key, snap in snaps.items():
        for net in ("actor", "critic"):
            for name, want in base[net].items():
                assert torch.equal(snap[net][name], want), f"{key}: {net}.{name}"
                n += 1
    assert n >= 4 * 10
