"""GPU tests for the SiLU + PPO-head fusions of the minibatch update
(silu_heads_fwd / heads_bwd_silu in stoix_amd/ops/csrc/mlp.hip) and their
wiring in the fused engine (STOIX_FUSED_HEADS)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

U16 = 2.0 ** -8   # bf16 unit roundoff (8 significant bits, round to nearest)
U32 = 2.0 ** -24  # fp32 unit roundoff

SHAPES = [(H, S) for H in (128, 256, 512) for S in (16, 144)]


@pytest.fixture(scope="module")
def ext():
    from stoix_amd import ops

    e = ops.ext(required=True)
    assert e is not None
    return e


def _inputs(H, S):
    """Seeded, non-degenerate operands of both kernels."""
    g = torch.Generator().manual_seed(1000 + H + S)
    r = lambda *s: torch.randn(*s, generator=g)
    bf = lambda t: t.bfloat16().cuda()
    return dict(
        Z2=bf(2.0 * r(2, S, H)),
        Wh=bf(r(16, H) / math.sqrt(H)),
        bh=bf(0.5 * r(16) + 0.25),
        Wv=bf(r(H) / math.sqrt(H)),
        bv=bf(0.5 * r(1) + 0.25),
        dhead=bf(r(S, 16)),
        dv=bf(r(S, 1)),
    )


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device="cuda")


@requires_gpu
@pytest.mark.parametrize("H,S", SHAPES)
def test_silu_heads_fwd(ext, H, S):
    """H2 is bit-equal to silu_fwd; every head / value element is within one
    bf16 rounding plus an fp32 accumulation (any order) of the fp64 product
    of the bf16 H2 with the weights plus the bf16 bias. The hipBLASLt addmm
    the kernel replaces has to meet the same bound."""
    x = _inputs(H, S)
    H2, heads, vpred = _nan(2, S, H), _nan(S, 16), _nan(S, 1)
    ext.silu_heads_fwd(x["Z2"], x["Wh"], x["bh"], x["Wv"], x["bv"], H2, heads,
                       vpred)
    H2_ref = _nan(2, S, H)
    ext.silu_fwd(x["Z2"], H2_ref)
    torch.cuda.synchronize()
    assert torch.equal(H2.view(torch.int16), H2_ref.view(torch.int16))

    heads_p, vpred_p = _nan(S, 16), _nan(S, 1)
    torch.addmm(x["bh"], H2_ref[0], x["Wh"].t(), out=heads_p)
    torch.addmm(x["bv"], H2_ref[1], x["Wv"].view(H, 1), out=vpred_p)

    d = lambda t: t.double()
    cases = {
        "heads": (d(H2_ref[0]), d(x["Wh"]).t(), d(x["bh"]), heads, heads_p),
        "vpred": (d(H2_ref[1]), d(x["Wv"]).view(H, 1), d(x["bv"]), vpred,
                  vpred_p),
    }
    for name, (h, w, b, fused, parent) in cases.items():
        T = h @ w + b
        bound = U16 * T.abs() + 2 * (H + 2) * U32 * (h.abs() @ w.abs())
        for tag, out in (("fused", fused), ("parent", parent)):
            err = (d(out) - T).abs()
            worst = (err / bound).max().item()
            print(f"{name} {tag} H={H} S={S}: max err/bound {worst:.3f}")
            assert torch.isfinite(d(out)).all(), f"{name} {tag}: not written"
            assert (err <= bound).all(), f"{name} {tag}: err/bound {worst:.3f}"


@requires_gpu
@pytest.mark.parametrize("H,S", SHAPES)
def test_silu_heads_fwd_without_value_head(ext, H, S):
    """With an empty vpred (the engine's default: the value head stays a
    library GEMM) H2 and heads are bit-equal to the full call's."""
    x = _inputs(H, S)
    H2, heads, vpred = _nan(2, S, H), _nan(S, 16), _nan(S, 1)
    ext.silu_heads_fwd(x["Z2"], x["Wh"], x["bh"], x["Wv"], x["bv"], H2, heads,
                       vpred)
    H2_b, heads_b = _nan(2, S, H), _nan(S, 16)
    ext.silu_heads_fwd(x["Z2"], x["Wh"], x["bh"], x["Wv"], x["bv"], H2_b,
                       heads_b, vpred[:0])
    torch.cuda.synchronize()
    assert torch.equal(H2.view(torch.int16), H2_b.view(torch.int16))
    assert torch.equal(heads.view(torch.int16), heads_b.view(torch.int16))


@requires_gpu
@pytest.mark.parametrize("H,S", SHAPES)
def test_heads_bwd_silu(ext, H, S):
    """dZ2 against the path it replaces on identical inputs (torch.mm into a
    bf16 dH2, then silu_bwd). Actor rows may differ by a one-ulp flip of the
    bf16 dH2 element (summation order) carried through one more rounding,
    plus the fp32 accumulation floor where the 16 products cancel. The
    critic's dH2 element is ONE product of two bf16 values, exact in fp32 and
    rounded once in both paths, so that half is bit-equal."""
    x = _inputs(H, S)
    dZ2 = _nan(2, S, H)
    ext.heads_bwd_silu(x["dhead"], x["dv"], x["Wh"], x["Wv"], x["Z2"], dZ2)
    dH2, dZ2_p = _nan(2, S, H), _nan(2, S, H)
    torch.mm(x["dhead"], x["Wh"], out=dH2[0])
    torch.mm(x["dv"], x["Wv"].view(1, H), out=dH2[1])
    ext.silu_bwd(dH2, x["Z2"], dZ2_p)
    torch.cuda.synchronize()

    d = lambda t: t.double()
    z = d(x["Z2"])
    s = torch.sigmoid(z)
    grad = (s * (1 + z * (1 - s))).abs()
    sums = (
        d(x["dhead"]).abs() @ d(x["Wh"]).abs(),
        (d(x["dv"]) * d(x["Wv"]).view(1, H)).abs(),
    )
    assert torch.isfinite(d(dZ2)).all(), "dZ2 not fully written"
    for net, name in enumerate(("actor", "critic")):
        p = d(dZ2_p[net])
        err = (d(dZ2[net]) - p).abs()
        bound = 2.0 ** -6 * p.abs() + grad[net] * 36 * U32 * sums[net]
        ndiff = int((dZ2[net].view(torch.int16) != dZ2_p[net].view(torch.int16)).sum())
        ok = err <= bound
        print(f"{name} H={H} S={S}: {ndiff}/{p.numel()} elements differ, "
              f"{int((~ok).sum())} outside the bound")
        assert ok.all(), f"{name}: {int((~ok).sum())} elements outside the bound"
        if net == 1:
            assert ndiff == 0, f"critic: {ndiff} elements not bit-equal"


@requires_gpu
def test_fused_heads_reject_unsupported_shapes(ext):
    """S must be whole 16-row tiles and HID an instantiated width."""
    for H, S, msg in ((256, 24, "S % 16 == 0"), (192, 16, "HID 128/256/512")):
        Z2 = torch.zeros(2, S, H, dtype=torch.bfloat16, device="cuda")
        z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="cuda")
        with pytest.raises(RuntimeError, match=msg):
            ext.silu_heads_fwd(Z2, z(16, H), z(16), z(H), z(1), z(2, S, H),
                               z(S, 16), z(S, 1))
        with pytest.raises(RuntimeError, match=msg):
            ext.heads_bwd_silu(z(S, 16), z(S, 1), z(16, H), z(H), Z2,
                               z(2, S, H))


# ------------------------------------------------------------------ engine


def _learner(config, overrides, heads=None):
    """A PPOLearner; `heads` sets STOIX_FUSED_HEADS for the construction of
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
         "system.epochs=1", "system.ent_coef=0.0", "logger.loggers=[]"]
        + overrides,
    )
    cfg.arch.n_devices = 1
    check_total_timesteps(cfg)
    device = torch.device("cuda:0")
    with pytest.MonkeyPatch.context() as mp:
        if heads is not None:
            mp.setenv("STOIX_FUSED_HEADS", heads)
        torch.manual_seed(11)
        env = environments.make_single(cfg, 256, device, seed=3)
        learner = PPOLearner(cfg, env, device)
    if heads is not None:
        assert learner.fused is not None
        assert learner.fused.fused_heads == (heads != "0")
        assert learner.fused.fused_vpred == (heads == "2")
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
            out[f"{tag}.{name}"] = gview.float().flatten().clone()
    return out


def _rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def ant_three_way(ext):
    """The learner of test_fused_vs_eager_gradients_one_minibatch three ways
    on identical rollout buffers: eager fp32, fused with the head fusions
    off, fused with them on (knob 1, the default: value head on the library
    GEMM) and fully on (knob 2: value head fused too). Returns per tensor
    (r, e, r2): r = |g_on - g_off| / |g_off|, r2 the same for knob 2,
    e = |g_off - g_eager| / |g_eager|."""
    cont = "default/anakin/default_ff_ppo_continuous.yaml"
    ant = ["env=brax/ant"]
    off = _learner(cont, ant + ["system.compute_dtype=bf16"], heads="0")
    on = _learner(cont, ant + ["system.compute_dtype=bf16"], heads="1")
    on2 = _learner(cont, ant + ["system.compute_dtype=bf16"], heads="2")
    eager = _learner(cont, ant + ["system.compute_dtype=fp32", "system.fused=false"])
    assert eager.fused is None
    _share_rollout(off, [on, on2, eager])

    TB = eager.T * eager.B
    obs = eager.buf_obs.view(TB, -1)
    act = eager.buf_action.view(TB, -1)
    from stoix_amd.ops.losses import clipped_value_loss, ppo_clip_loss

    a_loss = ppo_clip_loss(eager.actor(obs).log_prob(act),
                           eager.buf_log_prob.view(TB), eager.buf_adv.view(TB),
                           float(eager.sys.clip_eps))
    v_loss = clipped_value_loss(eager.critic(obs), eager.buf_value.view(TB),
                                eager.buf_targets.view(TB),
                                float(eager.sys.clip_eps))
    (a_loss + float(eager.sys.vf_coef) * v_loss).backward()

    g_off, g_on, g_on2 = _fused_grads(off), _fused_grads(on), _fused_grads(on2)
    OBS, H, K1P = off.fused.OBS, off.fused.H, off.fused.K1P
    al = [m for m in eager.actor.torso.net if hasattr(m, "weight")]
    cl = [m for m in eager.critic.torso.net if hasattr(m, "weight")]
    head = eager.actor.action_head
    w1 = lambda g: g.view(H, K1P)[:, :OBS].flatten()
    # name -> (selector into the fused tensor, eager gradient)
    pairs = {
        "a.W1": ("a.W1", w1, al[0].weight.grad),
        "a.b1": ("a.b1", None, al[0].bias.grad),
        "a.W2": ("a.W2", None, al[1].weight.grad),
        "a.b2": ("a.b2", None, al[1].bias.grad),
        "a.Wloc": ("a.Wh", lambda g: g[: 8 * H], head.loc.weight.grad),
        "a.Wscale": ("a.Wh", lambda g: g[8 * H :], head.scale.weight.grad),
        "c.W1": ("c.W1", w1, cl[0].weight.grad),
        "c.b1": ("c.b1", None, cl[0].bias.grad),
        "c.W2": ("c.W2", None, cl[1].weight.grad),
        "c.b2": ("c.b2", None, cl[1].bias.grad),
        "c.Wv": ("c.Wv", None, eager.critic.critic_head.linear.weight.grad),
    }
    out = {}
    for name, (key, sel, ge) in pairs.items():
        sel = sel or (lambda g: g)
        out[name] = (_rel(sel(g_on[key]), sel(g_off[key])),
                     _rel(sel(g_off[key]), ge.float().flatten()),
                     _rel(sel(g_on2[key]), sel(g_off[key])))
    return out


@requires_gpu
def test_fused_heads_engine_gradients_ant(ant_three_way):
    """Summation-order differences sit well inside the bf16 path's own
    distance from fp32: r <= e / 4 for every tensor (a layout bug gives
    r ~ 1)."""
    for name, (r, e, r2) in ant_three_way.items():
        print(f"ant {name}: r={r:.3e} r(knob 2)={r2:.3e} e={e:.3e}")
    for name, (r, e, r2) in ant_three_way.items():
        assert r <= e / 4, f"{name}: r={r:.3e} e={e:.3e}"
        assert r2 <= e / 4, f"{name}: knob 2 r={r2:.3e} e={e:.3e}"


@requires_gpu
def test_fused_heads_engine_gradients_cartpole(ant_three_way):
    """The discrete engine, fusions on against off. It has no eager leg, so
    r is set against the continuous case's e of the same tensor (the head
    against the smaller of its loc / scale halves)."""
    disc = "default/anakin/default_ff_ppo.yaml"
    over = ["env=classic/cartpole", "system.compute_dtype=bf16"]
    off = _learner(disc, over, heads="0")
    on = _learner(disc, over, heads="1")
    assert off.fused.discrete and on.fused.discrete
    _share_rollout(off, [on])
    g_off, g_on = _fused_grads(off), _fused_grads(on)
    e = {k: v[1] for k, v in ant_three_way.items()}
    e["a.Wh"] = min(e["a.Wloc"], e["a.Wscale"])
    rs = {k: _rel(g_on[k], g_off[k]) for k in g_off if k in e}
    assert {"a.W1", "a.W2", "a.Wh", "c.W1", "c.W2", "c.Wv"} <= set(rs)
    for name, r in rs.items():
        print(f"cartpole {name}: r={r:.3e} e(ant)={e[name]:.3e}")
    for name, r in rs.items():
        assert r <= e[name] / 4, f"{name}: r={r:.3e} e={e[name]:.3e}"
