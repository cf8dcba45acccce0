"""GPU tests for the pipelined, paired split-K wgrad kernel and the paired
slab reduce (wgrad_pair_kernel / slab_reduce_pair_kernel in
stoix_amd/ops/csrc/wgrad.hip) and their wiring in the fused PPO engine
(STOIX_FUSED_WGRAD). The contract is the summation order: every slab
element is the same fp32 value the old wgrad_kernel writes."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

U16 = 2.0 ** -8   # bf16 unit roundoff (8 significant bits, round to nearest)
U32 = 2.0 ** -24  # fp32 unit roundoff


@pytest.fixture(scope="module")
def ext():
    from stoix_amd import ops

    e = ops.ext(required=True)
    assert e is not None
    return e


def _n_slices(S):
    n = 64
    while n > 4 and S % (32 * n) != 0:
        n //= 2
    return n


@functools.lru_cache(maxsize=None)
def _operands(N, K, S, shared_x):
    """Seeded operands, different for the two nets (X shared for the K1P
    shapes, as the engine passes one Xmb for both). Never written to."""
    g = torch.Generator().manual_seed(7000 + 13 * N + 5 * K + S)
    dZ = [(torch.randn(S, N, generator=g) * 0.1).bfloat16().cuda() for _ in range(2)]
    X0 = torch.randn(S, K, generator=g).bfloat16().cuda()
    X1 = X0 if shared_x else torch.randn(S, K, generator=g).bfloat16().cuda()
    return dZ, [X0, X1]


def _layout(K, NV):
    """Different dW/db offsets per net, gaps between the ranges, and a slab
    stride larger than the used range."""
    dW = [8, 40]
    db = [8 + NV[0] * K + 24, 40 + NV[1] * K + 8]
    stride = max(db[0] + NV[0], db[1] + NV[1]) + 64
    return dW, db, stride


def _slabs(stride, fill):
    return [torch.full((64, stride), fill, dtype=torch.float32, device="cuda")
            for _ in range(2)]


def _run_old(ext, dZ, X, slabs, dW, db, NV):
    for i in range(2):
        ext.wgrad(dZ[i], X[i], slabs[i], dW[i], db[i], NV[i])


def _run_pair(ext, dZ, X, slabs, dW, db, NV):
    return ext.wgrad_pair(dZ[0], X[0], slabs[0], dW[0], db[0], NV[0],
                          dZ[1], X[1], slabs[1], dW[1], db[1], NV[1])


WIDE = [(256, 256, (256, 256)), (256, 32, (256, 256)), (256, 96, (256, 256)),
        (16, 256, (16, 1))]
OTHER = [(128, 128, (128, 128)), (512, 512, (512, 512)), (512, 128, (512, 512)),
         (16, 128, (16, 1)), (16, 512, (16, 1))]
CASES = ([(N, K, NV, S) for (N, K, NV) in WIDE for S in (128, 384, 2048, 4096, 6144)]
         + [(N, K, NV, S) for (N, K, NV) in OTHER for S in (384, 6144)])


@requires_gpu
@pytest.mark.parametrize("N,K,NV,S", CASES)
def test_pair_slab_images_bit_equal(ext, N, K, NV, S):
    """Before any reduce: every element the old kernel writes holds the same
    fp32 bits in the new slab, and every element it leaves alone (rows >=
    N_VALID, images >= n_slices, floats outside the dW and db ranges) is
    still the NaN the new slab was filled with."""
    dZ, X = _operands(N, K, S, K <= 128 and N != 16)
    dW, db, stride = _layout(K, NV)
    old, new = _slabs(stride, 0.0), _slabs(stride, float("nan"))
    _run_old(ext, dZ, X, old, dW, db, NV)
    assert _run_pair(ext, dZ, X, new, dW, db, NV) is True
    torch.cuda.synchronize()
    ns = _n_slices(S)
    for i in range(2):
        written = torch.zeros(64, stride, dtype=torch.bool, device="cuda")
        written[:ns, dW[i]: dW[i] + NV[i] * K] = True
        written[:ns, db[i]: db[i] + NV[i]] = True
        assert (old[i][~written] == 0).all(), "mask misses an old-kernel write"
        assert torch.equal(new[i][written].view(torch.int32),
                           old[i][written].view(torch.int32)), f"net {i}"
        assert torch.isnan(new[i][~written]).all(), f"net {i}: stray write"


def _reduce_old(ext, slabs, stride):
    out = []
    for s in slabs:
        g = torch.zeros(stride, dtype=torch.bfloat16, device="cuda")
        ext.slab_reduce(s, g, torch.zeros(0, device="cuda"),
                        torch.zeros(0, dtype=torch.int64, device="cuda"))
        out.append(g)
    return out


def _reduce_pair(ext, slabs, stride, sq=None, st=None):
    gs = [torch.zeros(stride, dtype=torch.bfloat16, device="cuda") for _ in range(2)]
    sq = sq or [torch.zeros(0, device="cuda")] * 2
    st = st or [torch.zeros(0, dtype=torch.int64, device="cuda")] * 2
    ext.slab_reduce_pair(slabs[0], gs[0], sq[0], st[0], slabs[1], gs[1], sq[1], st[1])
    return gs


@requires_gpu
@pytest.mark.parametrize("N,K,NV", [(256, 256, (256, 256)), (256, 32, (256, 256)),
                                    (16, 256, (16, 1))])
def test_pair_matches_fp64(ext, N, K, NV):
    """Independent of the old kernel: reduced dW and db are within one bf16
    rounding plus an fp32 accumulation in any order of the fp64 product of
    the bf16 operands. The old path has to meet the same bound."""
    S = 4096
    dZ, X = _operands(N, K, S, K <= 128 and N != 16)
    dW, db, stride = _layout(K, NV)
    new, old = _slabs(stride, 0.0), _slabs(stride, 0.0)
    _run_pair(ext, dZ, X, new, dW, db, NV)
    _run_old(ext, dZ, X, old, dW, db, NV)
    paths = {"pair": _reduce_pair(ext, new, stride),
             "old": _reduce_old(ext, old, stride)}
    torch.cuda.synchronize()
    for i in range(2):
        z, x = dZ[i].double(), X[i].double()
        T = (z.t() @ x)[: NV[i]]
        A = (z.abs().t() @ x.abs())[: NV[i]]
        Tb = z.sum(0)[: NV[i]]
        Ab = z.abs().sum(0)[: NV[i]]
        bw = U16 * T.abs() + 2 * (S + 2) * U32 * A
        bb = U16 * Tb.abs() + 2 * (S + 2) * U32 * Ab
        for name, gs in paths.items():
            gw = gs[i][dW[i]: dW[i] + NV[i] * K].view(NV[i], K).double()
            gb = gs[i][db[i]: db[i] + NV[i]].double()
            ew, eb = (gw - T).abs(), (gb - Tb).abs()
            print(f"{name} net {i}: max err/bound dW {(ew / bw).max().item():.3f} "
                  f"db {(eb / bb).max().item():.3f}")
            assert (ew <= bw).all(), f"{name} net {i}: dW outside the bound"
            assert (eb <= bb).all(), f"{name} net {i}: db outside the bound"


@requires_gpu
def test_slab_reduce_pair(ext):
    """Bit-equal to two slab_reduce calls on copies, slabs left untouched,
    Adam prologue once per chain; and no staleness: a second pair + reduce
    on the same (un-zeroed) slabs with different operands equals a run on
    fresh zero slabs."""
    N, K, NV, S = 256, 256, (256, 256), 4096
    dZ, X = _operands(N, K, S, False)
    dW, db, stride = _layout(K, NV)
    slabs = _slabs(stride, 0.0)
    _run_pair(ext, dZ, X, slabs, dW, db, NV)
    before = [s.clone() for s in slabs]
    ref = _reduce_old(ext, [s.clone() for s in slabs], stride)
    sq = [torch.full((3,), 5.0, device="cuda") for _ in range(2)]
    st = [torch.full((1,), 7 + i, dtype=torch.int64, device="cuda") for i in range(2)]
    got = _reduce_pair(ext, slabs, stride, sq, st)
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(got[i].view(torch.int16), ref[i].view(torch.int16))
        assert torch.equal(slabs[i].view(torch.int32), before[i].view(torch.int32))
        assert sq[i].tolist() == [0.0, 5.0, 5.0]
        assert st[i].item() == 8 + i
    # second minibatch on the same slabs: other operands (the nets swapped
    # and a different X), against fresh zero slabs
    dZ2, X2 = [dZ[1], dZ[0]], [X[1], X[0]]
    _run_pair(ext, dZ2, X2, slabs, dW, db, NV)
    again = _reduce_pair(ext, slabs, stride)
    fresh = _slabs(stride, 0.0)
    _run_pair(ext, dZ2, X2, fresh, dW, db, NV)
    want = _reduce_pair(ext, fresh, stride)
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(again[i].view(torch.int16), want[i].view(torch.int16))
        assert not torch.equal(again[i].view(torch.int16), got[i].view(torch.int16))


@requires_gpu
def test_pair_rejections_and_fallback(ext):
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
    S, N, K = 256, 256, 32
    slab = lambda: torch.zeros(64, N * K + N, device="cuda")
    call = lambda dZ0, X0, dZ1, X1: ext.wgrad_pair(
        dZ0, X0, slab(), 0, N * K, N, dZ1, X1, slab(), 0, N * K, N)
    with pytest.raises(RuntimeError, match="dtype"):
        call(z(S, N).float(), z(S, K), z(S, N), z(S, K))
    with pytest.raises(RuntimeError, match="contiguous"):
        call(z(N, S).t(), z(S, K), z(S, N), z(S, K))
    with pytest.raises(RuntimeError, match="multiple of 128"):
        call(z(96, N), z(96, K), z(96, N), z(96, K))
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ext.wgrad_pair(z(S, N), z(S, 48), torch.zeros(64, N * 48 + N, device="cuda"),
                       0, N * 48, N, z(S, N), z(S, 48),
                       torch.zeros(64, N * 48 + N, device="cuda"), 0, N * 48, N)
    with pytest.raises(RuntimeError, match="row mismatch"):
        call(z(S, N), z(S + 128, K), z(S, N), z(S, K))
    with pytest.raises(RuntimeError, match="row mismatch"):
        call(z(S, N), z(S, K), z(S + 128, N), z(S + 128, K))
    # H = 384 is outside {128, 256, 512}: the old kernels' result, bit for
    # bit, not a neighbouring instantiation's
    N = K = 384
    NV, S = (N, N), 384
    dZ, X = _operands(N, K, S, False)
    dW, db, stride = _layout(K, NV)
    old, new = _slabs(stride, 0.0), _slabs(stride, float("nan"))
    _run_old(ext, dZ, X, old, dW, db, NV)
    assert _run_pair(ext, dZ, X, new, dW, db, NV) is False
    torch.cuda.synchronize()
    for i in range(2):
        written = ~torch.isnan(new[i])
        assert written.sum().item() == 4 * (N * K + N)
        assert (old[i][~written] == 0).all()
        assert torch.equal(new[i][written].view(torch.int32),
                           old[i][written].view(torch.int32))


def _small():
    """S=128, N_STRIDE=16, K=32 operands and the [64, 16*32+16] zero slab of
    the single-net argument tests: dW at 0, db right behind it, nothing to
    spare."""
    S, N, K = 128, 16, 32
    g = torch.Generator().manual_seed(4242)
    dZ = (torch.randn(S, N, generator=g) * 0.1).bfloat16().cuda()
    X = torch.randn(S, K, generator=g).bfloat16().cuda()
    slab = torch.zeros(64, N * K + N, dtype=torch.float32, device="cuda")
    return S, N, K, dZ, X, slab


@requires_gpu
@pytest.mark.parametrize("case", ["dW_past_stride", "db_past_stride", "x_rows"])
def test_wgrad_refuses_out_of_range(ext, case):
    """wgrad() runs wgrad_pair()'s operand and slab-range checks: a dW or db
    range that ends past the slab stride, or an X with other rows than dZ,
    raises in the binding, and nothing was launched: the slab is untouched."""
    S, N, K, dZ, X, slab = _small()
    if case == "dW_past_stride":
        args, msg = (dZ, X, slab, N + 1, -1, N), "dW range"
    elif case == "db_past_stride":
        args, msg = (dZ, X, slab, 0, N * K + 1, N), "db range"
    else:
        X2 = torch.cat([X, X])
        args, msg = (dZ, X2, slab, 0, N * K, N), "row mismatch"
    with pytest.raises(RuntimeError, match=msg):
        ext.wgrad(*args)
    torch.cuda.synchronize()
    assert (slab == 0).all()


@requires_gpu
def test_slab_reduce_refuses_long_grad(ext):
    """slab_reduce() runs slab_reduce_pair()'s checks: a grad16 longer than a
    slab image raises before any launch."""
    _, _, _, _, _, slab = _small()
    grad16 = torch.zeros(slab.size(1) + 1, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="longer than a slab image"):
        ext.slab_reduce(slab, grad16, torch.zeros(0, device="cuda"),
                        torch.zeros(0, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    assert (slab == 0).all() and (grad16 == 0).all()


@requires_gpu
def test_wgrad_in_range_equals_pair_fallback(ext):
    """In-range offsets at the same shape still go through: wgrad() fills the
    slab bit for bit as wgrad_pair()'s fallback does (K = 32 with a 16-wide
    dZ is outside the paired table, so the fallback is the same kernel)."""
    S, N, K, dZ, X, slab = _small()
    ext.wgrad(dZ, X, slab, 0, N * K, N)
    pair = [torch.zeros_like(slab) for _ in range(2)]
    assert ext.wgrad_pair(dZ, X, pair[0], 0, N * K, N,
                          dZ, X, pair[1], 0, N * K, N) is False
    torch.cuda.synchronize()
    assert slab[:4].abs().sum().item() > 0 and (slab[4:] == 0).all()
    for p in pair:
        assert torch.equal(p.view(torch.int32), slab.view(torch.int32))


# ------------------------------------------------------------------ engine


def _learner(config, overrides, wgrad):
    """A PPOLearner; `wgrad` sets STOIX_FUSED_WGRAD for the construction of
    its fused engine (the knob is read there)."""
    from stoix_amd import envs as environments
    from stoix_amd.config import compose
    from stoix_amd.systems.ppo.ff_ppo import PPOLearner
    from stoix_amd.utils.total_timestep_checker import check_total_timesteps

    cfg = compose(
        config,
        ["arch.total_num_envs=256", "arch.total_timesteps=null",
         "arch.num_updates=4", "arch.num_evaluation=1", "arch.seed=11",
         "system.rollout_length=16", "system.num_minibatches=1",
         "system.epochs=1", "system.ent_coef=0.0", "logger.loggers=[]",
         "system.compute_dtype=bf16"]
        + overrides,
    )
    cfg.arch.n_devices = 1
    check_total_timesteps(cfg)
    device = torch.device("cuda:0")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("STOIX_FUSED_WGRAD", wgrad)
        torch.manual_seed(11)
        env = environments.make_single(cfg, 256, device, seed=3)
        learner = PPOLearner(cfg, env, device)
    assert learner.fused is not None
    assert learner.fused.fused_wgrad == (wgrad != "0")
    return learner


BUFFERS = ["buf_obs", "buf_action", "buf_log_prob", "buf_value",
           "buf_bootstrap", "buf_reward", "buf_discount", "buf_adv",
           "buf_targets"]


def _share_rollout(src, others):
    """One rollout of `src`, copied with its parameters into `others`, and
    the identity permutation everywhere."""
    src.rollout_phase()
    snap = src.snapshot_params()
    perm = torch.arange(src.T * src.B, device=src.device)
    src.perm_buf.copy_(perm)
    for o in others:
        o.load_params(snap)
        for name in BUFFERS:
            getattr(o, name).copy_(getattr(src, name))
        o.perm_buf.copy_(perm)


def _fused_grads(learner):
    """One minibatch of the fused update; its bf16 gradients by tensor."""
    learner.epoch_phase()
    torch.cuda.synchronize()
    F_ = learner.fused
    out = {}
    for tag, chain in (("a", F_.actor_chain), ("c", F_.critic_chain)):
        for name, gview in chain.gviews16.items():
            out[f"{tag}.{name}"] = gview.clone()
    return out


@requires_gpu
@pytest.mark.parametrize("config,env", [
    ("default/anakin/default_ff_ppo_continuous.yaml", "brax/ant"),
    ("default/anakin/default_ff_ppo.yaml", "classic/cartpole"),
])
def test_engine_gradients_bit_equal(ext, config, env):
    """STOIX_FUSED_WGRAD=0 against =1 on identical rollout buffers: every
    gradient tensor of both chains is bit-equal, and still is after a second
    epoch_phase() (the un-zeroed slab across minibatches)."""
    off = _learner(config, [f"env={env}"], "0")
    on = _learner(config, [f"env={env}"], "1")
    _share_rollout(off, [on])
    for rnd in range(2):
        g_off, g_on = _fused_grads(off), _fused_grads(on)
        assert set(g_off) == set(g_on) and len(g_off) >= 8
        for name in ("a.W1", "a.W2", "a.Wh", "c.W1", "c.W2", "c.Wv"):
            assert g_off[name].float().abs().sum().item() > 0, f"{name}: zero"
        for name in g_off:
            assert torch.equal(g_on[name].view(torch.int16),
                               g_off[name].view(torch.int16)), \
                f"epoch {rnd} {name}: not bit-equal"
