"""GPU tests for linear_silu_heads_pair (l2_fwd_heads_kernel in
stoix_amd/ops/csrc/mlp.hip): the layer-2 Linear + SiLU + heads of both nets in
one launch with W2 held in LDS, and its wiring in the fused engine
(STOIX_FUSED_L2). The Z2 test prints, per shape, whether Z2 was bit-equal to
the hipBLASLt addmm and the kernel/library error ratio against fp64."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

U16 = 2.0 ** -8   # bf16 unit roundoff (8 significant bits, round to nearest)
U32 = 2.0 ** -24  # fp32 unit roundoff

# Largest error of the kernel over largest error of the library, both against
# fp64 in units of `_z2_bound`. Either path is an fp32 accumulation and ONE
# bf16 rounding, so over thousands of elements both maxima sit at the
# rounding's half ulp and the ratio is 1 up to the fp32 floor; torch's CPU
# bf16 addmm on these inputs reaches 0.946-0.984 of the bound over the shapes
# here (and an fp32 matmul rounded once gives the same maxima, ratio 1.0000),
# which leaves a path that stays inside the bound a ratio of at most
# 1 / 0.946 = 1.057.
Z2_FACTOR = 1.06

# 32896 = 128 rows more than the 128 workgroups x 8 waves x 32 rows a
# 256-CU device's grid covers in its first pass: some waves walk a 2nd tile
OP_SHAPES = [(H, S) for H in (128, 256) for S in (128, 384, 1280)] + [(128, 32896)]


@pytest.fixture(scope="module")
def ext():
    from stoix_amd import ops

    e = ops.ext(required=True)
    assert e is not None
    return e


def _inputs(H, S, seed=0):
    """Seeded random bf16 operands; biases large enough to matter."""
    g = torch.Generator().manual_seed(7000 + H + S + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    bf = lambda t: t.bfloat16().cuda()
    return dict(
        H1=bf(r(2, S, H)),
        W2=bf(r(2, H, H) / math.sqrt(H)),
        b2=bf(0.5 * r(2, H)),
        Wh=bf(r(16, H) / math.sqrt(H)),
        bh=bf(0.5 * r(16) + 0.25),
        Wv=bf(r(H) / math.sqrt(H)),
        bv=bf(0.5 * r(1) + 0.25),
    )


def _fill(*shape):
    """Sentinel buffers: -3.5 is a bf16 value no output of these inputs is
    required to take, and a row of them is easy to recognise."""
    return torch.full(shape, -3.5, dtype=torch.bfloat16, device="cuda")


def _bits(t):
    return t.contiguous().view(torch.int16)


def _call(ext, x, Z2, H2, heads, vpred):
    return ext.linear_silu_heads_pair(
        x["H1"], x["W2"][0], x["b2"][0], x["W2"][1], x["b2"][1], x["Wh"],
        x["bh"], x["Wv"], x["bv"], Z2, H2, heads, vpred)


def _library_z2(x):
    S, H = x["H1"].shape[1:]
    Z2 = _fill(2, S, H)
    for n in (0, 1):
        torch.addmm(x["b2"][n], x["H1"][n], x["W2"][n].t(), out=Z2[n])
    return Z2


def _z2_bound(x):
    """fp64 Z2 and the elementwise bound of any fp32-accumulated, once-rounded
    result: half a bf16 ulp of the exact value (U16 |T|) plus an fp32
    accumulation of H products and the bias in any order."""
    d = lambda t: t.double()
    H = x["H1"].shape[2]
    T = torch.bmm(d(x["H1"]), d(x["W2"]).transpose(1, 2)) + d(x["b2"])[:, None]
    mag = torch.bmm(d(x["H1"]).abs(), d(x["W2"]).abs().transpose(1, 2)) \
        + d(x["b2"]).abs()[:, None]
    return T, U16 * T.abs() + 2 * (H + 2) * U32 * mag


@functools.lru_cache(maxsize=None)
def _op_case(H, S):
    """One run of the op and of the launches it replaces, shared by the
    op-level tests of a shape."""
    from stoix_amd import ops

    ext = ops.ext(required=True)
    x = _inputs(H, S)
    Z2, H2, heads = _fill(2, S, H), _fill(2, S, H), _fill(S, 16)
    took = _call(ext, x, Z2, H2, heads, heads[:0].view(-1))
    Z2_lib = _library_z2(x)
    torch.cuda.synchronize()
    return x, took, Z2, H2, heads, Z2_lib


@requires_gpu
@pytest.mark.parametrize("H,S", OP_SHAPES)
def test_h2_and_heads_are_the_old_kernels_of_its_own_z2(ext, H, S):
    """H2 given Z2 and heads given H2 are the repository's own order:
    silu_heads_fwd on the kernel's Z2 gives the same bytes."""
    x, took, Z2, H2, heads, _ = _op_case(H, S)
    assert took is True
    H2_old, heads_old = _fill(2, S, H), _fill(S, 16)
    ext.silu_heads_fwd(Z2, x["Wh"], x["bh"], x["Wv"], x["bv"], H2_old,
                       heads_old, heads_old[:0].view(-1))
    torch.cuda.synchronize()
    assert torch.equal(_bits(H2), _bits(H2_old))
    assert torch.equal(_bits(heads), _bits(heads_old))


@requires_gpu
@pytest.mark.parametrize("H,S", OP_SHAPES)
def test_z2_against_fp64_and_the_library(ext, H, S):
    """Z2 within the format bound of the fp64 product of the bf16 inputs, as
    the library's has to be; the two agree within one bf16 ulp of the exact
    value's binade (plus the fp32 floor where the products cancel); and the
    kernel's largest error is at most Z2_FACTOR times the library's."""
    x, took, Z2, _, _, Z2_lib = _op_case(H, S)
    assert took is True
    T, bound = _z2_bound(x)
    worst = {}
    for tag, out in (("kernel", Z2), ("library", Z2_lib)):
        err = (out.double() - T).abs()
        worst[tag] = (err / bound).max().item()
        print(f"Z2 {tag} H={H} S={S}: max err/bound {worst[tag]:.4f}")
        assert (err <= bound).all(), f"{tag}: err/bound {worst[tag]:.4f}"
    ulp = torch.exp2(torch.floor(torch.log2(T.abs().clamp_min(1e-30))) - 7)
    gap = (Z2.double() - Z2_lib.double()).abs()
    floor = bound - U16 * T.abs()
    assert (gap <= ulp + 2 * floor).all()
    n_diff = int((_bits(Z2) != _bits(Z2_lib)).sum())
    print(f"Z2 H={H} S={S}: bit-equal to the library: {n_diff == 0} "
          f"({n_diff} of {Z2.numel()} differ); "
          f"err ratio kernel/library {worst['kernel'] / worst['library']:.4f}")
    assert worst["kernel"] <= Z2_FACTOR * worst["library"]


@requires_gpu
@pytest.mark.parametrize("H,S", [(256, 384), (128, 128)])
def test_value_head_when_asked(ext, H, S):
    """With a vpred buffer the value head is the one silu_heads_fwd forms from
    the same Z2, and asking for it changes nothing else."""
    x, took, Z2, H2, heads, _ = _op_case(H, S)
    Z2_v, H2_v, heads_v, vpred = _fill(2, S, H), _fill(2, S, H), _fill(S, 16), _fill(S, 1)
    assert _call(ext, x, Z2_v, H2_v, heads_v, vpred) is True
    H2_old, heads_old, vpred_old = _fill(2, S, H), _fill(S, 16), _fill(S, 1)
    ext.silu_heads_fwd(Z2_v, x["Wh"], x["bh"], x["Wv"], x["bv"], H2_old,
                       heads_old, vpred_old)
    torch.cuda.synchronize()
    assert torch.equal(_bits(vpred), _bits(vpred_old))
    for a, b in ((Z2_v, Z2), (H2_v, H2), (heads_v, heads), (heads_v, heads_old)):
        assert torch.equal(_bits(a), _bits(b))


@requires_gpu
def test_categorical_head_width(ext):
    """ACT 16: every row of the 16-wide head tile carries a logit (no zero
    rows in Wh, no zero bias), exact against silu_heads_fwd."""
    H, S = 256, 128
    x = _inputs(H, S, seed=16)
    assert (x["Wh"].float().abs().sum(1) > 0).all() and (x["bh"] != 0).all()
    Z2, H2, heads = _fill(2, S, H), _fill(2, S, H), _fill(S, 16)
    assert _call(ext, x, Z2, H2, heads, heads[:0].view(-1)) is True
    H2_old, heads_old = _fill(2, S, H), _fill(S, 16)
    ext.silu_heads_fwd(Z2, x["Wh"], x["bh"], x["Wv"], x["bv"], H2_old,
                       heads_old, heads_old[:0].view(-1))
    torch.cuda.synchronize()
    assert torch.equal(_bits(heads), _bits(heads_old))
    assert (heads.float() != -3.5).all()


@requires_gpu
@pytest.mark.parametrize("H,S", [(512, 128), (256, 130)])
def test_refused_shapes_launch_nothing(ext, H, S):
    x = _inputs(H, S)
    outs = [_fill(2, S, H), _fill(2, S, H), _fill(S, 16), _fill(S, 1)]
    assert _call(ext, x, *outs) is False
    torch.cuda.synchronize()
    for o in outs:
        assert (o.float() == -3.5).all()


@requires_gpu
@pytest.mark.parametrize("H,S", [(256, 384), (128, 1280)])
def test_rows_past_s_stay_and_calls_repeat(ext, H, S):
    """Buffers with 128 more rows than S per net: the tails keep their
    sentinel. A second call on the same inputs gives the same bytes."""
    x = _inputs(H, S)
    big = [_fill(2 * S + 128, H), _fill(2 * S + 128, H), _fill(S + 128, 16),
           _fill(S + 128)]
    outs = [big[0][:2 * S].view(2, S, H), big[1][:2 * S].view(2, S, H),
            big[2][:S], big[3][:S]]
    assert _call(ext, x, *outs) is True
    again = [_fill(2, S, H), _fill(2, S, H), _fill(S, 16), _fill(S)]
    assert _call(ext, x, *again) is True
    torch.cuda.synchronize()
    for b, n in zip(big, (2 * S, 2 * S, S, S)):
        assert (b[n:].float() == -3.5).all()
    for a, b in zip(outs, again):
        assert torch.equal(_bits(a), _bits(b))
    _, _, Z2, H2, heads, _ = _op_case(H, S)
    for a, b in zip(outs[:3], (Z2, H2, heads)):
        assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ engine

def _learner(l2, hidden=256, num_envs=64, T=8, n_mb=2):
    """The small fused PPO learner of test_epoch_gather_engine_gpu (27 obs /
    8 act Ant, S = 256 rows), of the given width, built with the knob set."""
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
         "system.epochs=1", "logger.loggers=[]", "system.compute_dtype=bf16",
         f"network.actor_network.pre_torso.layer_sizes=[{hidden},{hidden}]",
         f"network.critic_network.pre_torso.layer_sizes=[{hidden},{hidden}]"],
    )
    cfg.arch.n_devices = 1
    check_total_timesteps(cfg)
    device = torch.device("cuda:0")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("STOIX_FUSED_L2", l2)
        mp.setenv("STOIX_FUSED_STRICT", "1")
        torch.manual_seed(11)
        env = environments.make_single(cfg, num_envs, device, seed=3)
        learner = PPOLearner(cfg, env, device)
    F_ = learner.fused
    assert F_ is not None and F_.H == hidden
    assert F_.fused_l2 == (l2 == "1")
    return learner


def _step(l2, hidden):
    learner = _learner(l2, hidden)
    learner.update_step()
    torch.cuda.synchronize()
    F_ = learner.fused
    grads = {"actor": F_.actor_chain.grad16.clone(),
             "critic": F_.critic_chain.grad16.clone()}
    return learner, learner.snapshot_params(), grads


@requires_gpu
def test_engine_update_step_with_and_without_the_knob():
    """One update step (S = 256, H = 256) from the same seed with the knob at
    0 and at 1. Where the op gives the library's Z2 bit for bit on the
    engine's own layer-2 operands every parameter is equal; otherwise the
    last minibatch's gradients agree at the tolerance of
    test_fused_gpu.test_fused_vs_eager_gradients_one_minibatch (cosine > 0.98,
    norm ratio within 15 %)."""
    import torch.nn.functional as TF

    off, p_off, g_off = _step("0", 256)
    on, p_on, g_on = _step("1", 256)
    F_ = on.fused
    assert F_.S == 256
    a16, c16 = F_.actor_chain.views16, F_.critic_chain.views16
    Z2 = torch.empty_like(F_.Z2)
    assert F_.ext.linear_silu_heads_pair(
        F_.H1, a16["W2"], a16["b2"], c16["W2"], c16["b2"], a16["Wh"],
        a16["bh"], c16["Wv"], c16["bv"], Z2, torch.empty_like(F_.H2),
        torch.empty_like(F_.heads), F_.no_vpred) is True
    Z2_lib = torch.empty_like(Z2)
    torch.addmm(a16["b2"], F_.H1[0], a16["W2"].t(), out=Z2_lib[0])
    torch.addmm(c16["b2"], F_.H1[1], c16["W2"].t(), out=Z2_lib[1])
    torch.cuda.synchronize()
    bit_equal = torch.equal(_bits(Z2), _bits(Z2_lib))
    print(f"engine operands: Z2 bit-equal to the library: {bit_equal}")
    n = 0
    for net in ("actor", "critic"):
        for name, want in p_off[net].items():
            got = p_on[net][name]
            assert torch.isfinite(got).all()
            if bit_equal:
                assert torch.equal(got, want), f"{net}.{name}"
            n += 1
        gf, ge = g_on[net].float(), g_off[net].float()
        cos = TF.cosine_similarity(gf, ge, dim=0).item()
        ratio = (gf.norm() / ge.norm().clamp_min(1e-12)).item()
        assert cos > 0.98 and abs(ratio - 1.0) < 0.15, f"{net}: {cos} {ratio}"
    assert n >= 10


@requires_gpu
def test_engine_keeps_the_old_launches_where_the_launcher_refuses():
    """H = 512: W2 does not fit in LDS, the launcher returns false, and the
    knob changes nothing: equal parameters after one update step."""
    off, p_off, _ = _step("0", 512)
    on, p_on, _ = _step("1", 512)
    F_ = on.fused
    a16, c16 = F_.actor_chain.views16, F_.critic_chain.views16
    assert F_.ext.linear_silu_heads_pair(
        F_.H1, a16["W2"], a16["b2"], c16["W2"], c16["b2"], a16["Wh"],
        a16["bh"], c16["Wv"], c16["bv"], torch.empty_like(F_.Z2),
        torch.empty_like(F_.H2), torch.empty_like(F_.heads),
        F_.no_vpred) is False
    for net in ("actor", "critic"):
        for name, want in p_off[net].items():
            assert torch.equal(p_on[net][name], want), f"{net}.{name}"
